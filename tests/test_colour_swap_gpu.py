"""Colour-swap augmentation of replay batches (xq_replay_set_colour_swap, DESIGN.md §4 "Colour-swap augmentation") on the device: the
staged batch against tests/colour_swap_ref.py bit for bit on every nibble of the board, the TD step on it against the existing step on
the host-swapped batch bit for bit (alone, behind n-step, with the mirror, under the legal-move bootstrap), the prioritized write-back,
off is off, the trainer, refusals, survival and the facade."""
import json
import subprocess

import numpy as np
import pytest

import batch_ref as br
import colour_swap_ref as cr
import mirror_ref as mr
import nstep_ref as nr
import xqoracle as xo
from test_dqn_gpu import CFG2_NET, make_net
from test_nstep_gpu import assert_assembled, filled, reference

pytestmark = pytest.mark.gpu

SMALL_NET = [1260, 64, 64, 8100]
GAMMA = 0.97
BATCHES = (1, 63, 64, 65, 257)
PER = (0.6, 0.4, 1e-3)
RING_SEED = 5                                   # (what test_nstep_gpu.filled gives its rings)


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


def assert_staged(got, want):
    for k in ("flags", "boards", "next_boards", "action", "slot"):
        assert np.array_equal(got[k], want[k]), k


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def same_step(a, b, batch):
    (qa, ya), (qb, yb) = a.last_td_values(batch), b.last_td_values(batch)
    assert np.array_equal(bits(qa), bits(qb)) and np.array_equal(bits(ya), bits(yb))
    (wa, ba), (wb, bb) = a.get_params(), b.get_params()
    assert np.array_equal(wa, wb) and np.array_equal(ba, bb)
    return wa


# ---- 1. every nibble ----------------------------------------------------------------------------------------------------------------
def nibble_fixture():
    """84 transitions that put every code 1..14 on every square of both boards, 15 squares at a time (the ring accepts at most 16
    pieces of one colour): code k on squares 15 j .. 15 j + 14 of the board, code 15 - k there on the next board; 90 with one piece each
    — code (s mod 14) + 1 on square s of the board and on square 89 - s of the next board, action s — so every action 0..89 is moved
    once; then 119 boards of 10 random pieces with actions that include -1 and 90..95.  293 slots: no multiple of the 64-row block."""
    rng = np.random.default_rng(77)
    n_rand = 119
    F, F2 = np.zeros((84, 90), np.uint8), np.zeros((84, 90), np.uint8)
    for k in range(1, 15):
        for j in range(6):
            F[(k - 1) * 6 + j, 15 * j:15 * j + 15] = k
            F2[(k - 1) * 6 + j, 15 * j:15 * j + 15] = 15 - k
    FA = (np.arange(84, dtype=np.int32) * 7) % 90
    S, S2 = np.zeros((90, 90), np.uint8), np.zeros((90, 90), np.uint8)
    for s in range(90):
        S[s, s] = s % 14 + 1
        S2[s, 89 - s] = s % 14 + 1
    A = np.arange(90, dtype=np.int32)
    RA = rng.integers(0, 90, size=n_rand).astype(np.int32)
    RA[:14] = [-1, 90, 91, 92, 93, 94, 95, -1, 0, 4, 8, 89, 81, 85]
    S = np.concatenate([F, S, nr.random_boards(rng, n_rand)])
    S2 = np.concatenate([F2, S2, nr.random_boards(rng, n_rand)])
    A = np.concatenate([FA, A, RA])
    order = rng.permutation(len(A))
    S, S2, A = S[order], S2[order], A[order]
    R = rng.uniform(-1.0, 1.0, size=len(A)).astype(np.float32)
    D = (rng.random(len(A)) < 0.15).astype(np.uint8)
    return dict(S=S, S2=S2, A=A, R=R, D=D, cap=len(A))


@pytest.mark.parametrize("prob", [1.0, 0.5])
def test_staged_batch_equals_the_reference_on_every_nibble(xq, small, prob):
    fx = nibble_fixture()
    for k in range(15):
        assert ((fx["S"] == k).any(axis=0)).all() and ((fx["S2"] == k).any(axis=0)).all()
    seed = 0xABCD00000000 + 41                                        # both key words in use
    rp = xq.ReplayBuffer(fx["cap"], seed=seed)
    try:
        rp.push(fx["S"], fx["A"], fx["R"], fx["D"], fx["S2"])
        assert rp.colour_swap() == (0.0, 0)
        rp.set_colour_swap(prob)
        moved = np.zeros((2, 90), bool)
        for call, batch in enumerate(BATCHES + (0,)):
            assert rp.colour_swap() == (prob, call) and rp.mirror == (0.0, 0)
            slots = rp.sample(batch) if batch else np.arange(fx["cap"], dtype=np.int32)
            small.td_grads_replay(rp, batch)
            small.apply_grads(0.0, 1.0)
            rows = len(slots)
            want = cr.stage(fx, slots, prob, call, seed)
            got = small.last_colour_swap(rows)
            assert_staged(got, want)
            if prob == 1.0:
                assert got["flags"].all()
            elif rows >= 63:
                assert got["flags"].any() and not got["flags"].all()
            m = got["flags"].astype(bool)
            assert np.array_equal(got["boards"][~m], fx["S"][slots][~m]) and np.array_equal(got["action"][~m], fx["A"][slots][~m])
            # the one-piece transitions, from the device's rows alone: the piece of a swapped row stands on (9 - row, col) in the other colour
            for i in np.flatnonzero(m & ((fx["S"][slots] != 0).sum(axis=1) == 1)):
                s = int(fx["A"][slots[i]])
                code = s % 14 + 1
                other = code + 7 if code <= 7 else code - 7
                sm, s2m = s + 81 - 18 * (s // 9), (89 - s) + 81 - 18 * ((89 - s) // 9)
                assert got["boards"][i, sm] == other and got["next_boards"][i, s2m] == other and got["action"][i] == sm
                assert (got["boards"][i] != 0).sum() == 1 and (got["next_boards"][i] != 0).sum() == 1
                moved[0, s] = moved[1, 89 - s] = True
        assert rp.colour_swap() == (prob, len(BATCHES) + 1) and rp.mirror == (0.0, 0)
        if prob == 1.0:
            assert moved.all()                    # the identity batch moved every square of both boards once
        # the ring was never written
        for s in (0, 17, fx["cap"] - 1):
            b, a, r, d, nb = rp.get(s)
            assert np.array_equal(b, fx["S"][s]) and np.array_equal(nb, fx["S2"][s]) and a == fx["A"][s]
    finally:
        rp.close()


# ---- 2. the step is the existing step on the staged batch ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,batch,extras,derive", [(SMALL_NET, 65, False, False), (CFG2_NET, 1024, False, False),
                                                       (CFG2_NET, 1024, True, False), (CFG2_NET, 1024, False, True)])
def test_step_is_the_existing_step_on_the_swapped_batch(xq, sizes, batch, extras, derive):
    lr = 0.05
    fx = nr.fixture(300, 4, 420, seed=11)
    rp = filled(xq, fx)
    a, w, b = make_net(xq, sizes, seed=8, gamma=GAMMA)
    bq, _, _ = make_net(xq, sizes, seed=8, gamma=GAMMA)
    try:
        for d in (a, bq):
            if extras:
                d.set_optimizer("adam")
                d.set_td_loss("huber", 0.05)
                d.set_grad_clip(1.0)
            if derive:
                d.set_l0_derive(True)
        rp.set_colour_swap(1.0)
        slots = rp.sample(batch)
        a.td_grads_replay(rp, batch)
        a.apply_grads(lr, 1.0 / batch)
        want = cr.stage(fx, slots, 1.0, 0, RING_SEED)
        assert_staged(a.last_colour_swap(batch), want)
        assert want["flags"].all() and ((want["action"] < 0).any() or batch < 1024)
        assert (want["action"] != fx["A"][slots]).any() and (want["boards"] != fx["S"][slots]).any()
        bq.td_update(want["boards"], want["next_boards"], want["action"], fx["R"][slots], fx["D"][slots], learning_rate=lr,
                     grad_scale=1.0 / batch)
        wa = same_step(a, bq, batch)
        assert np.abs(wa - w).max() > 0
        for refused in (lambda: a.last_n_step(1), lambda: a.last_mirror(1)):           # neither an n-step nor a mirror-mode step
            with pytest.raises(xq.XqError):
                refused()
    finally:
        a.close(); bq.close(); rp.close()


# ---- 3. with n-step -----------------------------------------------------------------------------------------------------------------
def test_colour_swap_behind_the_n_step_assembly(xq):
    n, batch, lr = 3, 257, 0.05
    fx = nr.fixture(300, 4, 420, seed=11)
    rp, plain = filled(xq, fx), filled(xq, fx)
    disc = nr.discounts(GAMMA, n)
    a, w, _ = make_net(xq, SMALL_NET, seed=8, gamma=GAMMA)
    p, _, _ = make_net(xq, SMALL_NET, seed=8, gamma=GAMMA)
    bq, _, _ = make_net(xq, SMALL_NET, seed=8, gamma=float(disc[n]))
    try:
        rp.set_colour_swap(0.5)
        rp.set_n_step(n, fx["stride"])
        plain.set_n_step(n, fx["stride"])
        assert rp.colour_swap() == (0.5, 0) and rp.n_step == (n, fx["stride"])
        slots = rp.sample(batch)
        assert np.array_equal(plain.sample(batch), slots)
        a.td_grads_replay(rp, batch)
        a.apply_grads(lr, 1.0 / batch)
        p.td_grads_replay(plain, batch)
        p.apply_grads(0.0, 1.0)
        ref = reference(fx, slots, n)
        S, A, R, D, S2 = nr.staged(fx, ref)
        want = cr.apply(S, A, S2, None, 0.5, 0, RING_SEED)
        want["slot"] = slots
        assert_staged(a.last_colour_swap(batch), want)
        assert ref["dead"].any() and (ref["steps"] == n).any() and want["flags"].any() and not want["flags"].all()
        got, without = a.last_n_step(batch), p.last_n_step(batch)
        for k in ("reward", "done", "steps", "first_slot", "last_slot"):
            assert np.array_equal(got[k], without[k]), k
        assert np.array_equal(got["action"], want["action"]) and np.array_equal(without["action"], ref["action"])
        assert_assembled(got, dict(ref, action=want["action"]))
        with pytest.raises(xq.XqError):
            p.last_colour_swap(1)
        bq.td_update(want["boards"], want["next_boards"], want["action"], R, D, learning_rate=lr, grad_scale=1.0 / batch)
        wa = same_step(a, bq, batch)
        assert np.abs(wa - w).max() > 0
    finally:
        a.close(); p.close(); bq.close(); rp.close(); plain.close()


# ---- 4. with the mirror -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prob,n", [(1.0, 1), (0.5, 1), (0.5, 3)])
def test_colour_swap_with_the_mirror_in_either_order(xq, prob, n):
    batch, lr = 257, 0.05
    fx = nr.fixture(300, 4, 420, seed=11)
    rp = filled(xq, fx)
    disc = nr.discounts(GAMMA, n)
    a, w, _ = make_net(xq, SMALL_NET, seed=8, gamma=GAMMA)
    bq, _, _ = make_net(xq, SMALL_NET, seed=8, gamma=float(disc[n]) if n > 1 else GAMMA)
    try:
        rp.set_mirror(prob)
        rp.set_colour_swap(prob)
        if n > 1:
            rp.set_n_step(n, fx["stride"])
        slots = rp.sample(batch)
        a.kernel_stats(2)
        a.td_grads_replay(rp, batch)
        a.apply_grads(lr, 1.0 / batch)
        st = {s["name"]: s["launches"] for s in a.kernel_stats()}
        assert st["mirror_stage"] == 1 and st["colour_swap_stage"] == 1 and ("nstep_assemble" in st) == (n > 1)
        a.kernel_stats(0)
        assert rp.mirror == (prob, 1) and rp.colour_swap() == (prob, 1)
        if n > 1:
            S, A, R, D, S2 = nr.staged(fx, reference(fx, slots, n))
        else:
            S, A, R, D, S2 = fx["S"][slots], fx["A"][slots], fx["R"][slots], fx["D"][slots], fx["S2"][slots]
        m1 = mr.apply(S, A, S2, prob, 0, RING_SEED)
        c1 = cr.apply(m1["boards"], m1["action"], m1["next_boards"], None, prob, 0, RING_SEED)
        c2 = cr.apply(S, A, S2, None, prob, 0, RING_SEED)
        m2 = mr.apply(c2["boards"], c2["action"], c2["next_boards"], prob, 0, RING_SEED)
        for k in ("boards", "next_boards", "action"):
            assert np.array_equal(c1[k], m2[k]), k                                 # the two commute
        gc, gm = a.last_colour_swap(batch), a.last_mirror(batch)
        assert_staged(gc, dict(c1, slot=slots))
        assert_staged(gm, dict(m2, slot=slots))
        assert np.array_equal(gc["flags"], c2["flags"]) and np.array_equal(gm["flags"], m1["flags"])
        if prob < 1.0:
            assert not np.array_equal(gc["flags"], gm["flags"])                    # two streams
            both, neither = (gc["flags"] & gm["flags"]).astype(bool), ~(gc["flags"] | gm["flags"]).astype(bool)
            assert both.any() and neither.any() and (gc["flags"] & ~gm["flags"] & 1).any() and (gm["flags"] & ~gc["flags"] & 1).any()
        bq.td_update(c1["boards"], c1["next_boards"], c1["action"], R, D, learning_rate=lr, grad_scale=1.0 / batch)
        wa = same_step(a, bq, batch)
        assert np.abs(wa - w).max() > 0
    finally:
        a.close(); bq.close(); rp.close()


# ---- 5. under the legal-move bootstrap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 2])
def test_colour_swap_under_the_legal_bootstrap(xq, golden_dir, rule):
    """a tracking ring of tests/test_legal_gpu.py's pool rows (ref_bigmoves and ref_sparse, both sides, sides without a move, done and
    dead rows), every row swapped: the image has the original's move counts for the other side, the staged side bytes are 1 - side, and
    the step is the sided host step on the host-swapped batch bit for bit"""
    from test_legal_gpu import legal_net, pool, rows_of
    rows, lr = 576, 0.05
    b = rows_of(pool(golden_dir), np.arange(rows))
    rp = xq.ReplayBuffer(rows, seed=RING_SEED)
    a, c = legal_net(xq, SMALL_NET), legal_net(xq, SMALL_NET)
    try:
        rp.track_next_player()
        rp.push(b["S"], b["A"], b["R"], b["D"], b["S2"], next_player=b["side"])
        rp.set_colour_swap(1.0)
        a.kernel_stats(2)
        a.td_grads_replay(rp, 0, td_net=rule)
        a.apply_grads(lr, 1.0 / rows)
        st = {s["name"]: s["launches"] for s in a.kernel_stats()}
        assert st["colour_swap_stage"] == 1 and "legal_side_stage" not in st and st["legal_qmax"] >= 1
        a.kernel_stats(0)
        fx = dict(S=b["S"], A=b["A"], S2=b["S2"])
        want = cr.stage(fx, np.arange(rows), 1.0, 0, RING_SEED, side=b["side"])
        got = a.last_colour_swap(rows, next_player=True)
        assert_staged(got, want)
        assert np.array_equal(got["next_player"], 1 - b["side"]) and set(np.unique(b["side"])) == {0, 1}
        skipped = (b["D"] != 0) | (b["A"] < 0)
        lens = np.array([len(x) for x in b["lists"]])
        La = a.last_legal(rows, z96=False)
        assert np.array_equal(La["n_moves"], np.where(skipped, -1, lens))
        assert skipped.any() and (lens[~skipped] == 0).any() and (lens[~skipped] > 40).any()
        c.td_update(want["boards"], want["next_boards"], want["action"], b["R"], b["D"], td_net=rule, learning_rate=lr,
                    grad_scale=1.0 / rows, next_player=want["next_player"])
        same_step(a, c, rows)
        Lc = c.last_legal(rows, z96=False)
        for k in ("n_moves", "a_star"):
            assert np.array_equal(La[k], Lc[k]), k
        assert np.array_equal(bits(La["zmax"]), bits(Lc["zmax"]))
        # half the rows, behind the mirror: the side byte is taken at the sampled slot, then flipped on the flagged rows
        rp.set_colour_swap(0.5)
        rp.set_mirror(0.5)
        slots = rp.sample(200)
        a.td_grads_replay(rp, 200, td_net=rule)
        a.apply_grads(0.0, 1.0)
        got = a.last_colour_swap(200, next_player=True)
        f = cr.flags(200, 0.5, 1, RING_SEED)
        assert np.array_equal(got["flags"], f) and np.array_equal(got["next_player"], np.where(f, 1 - b["side"][slots], b["side"][slots]))
    finally:
        a.close(); c.close(); rp.close()


# ---- 6. prioritized -----------------------------------------------------------------------------------------------------------------
def test_prioritized_swapped_td_step_and_its_priorities(xq):
    """a Double-DQN step of the small net on a prioritized draw with colour swap 0.5, against tests/batch_ref.py on the host-swapped
    batch (the bounds of tests/test_mirror_gpu.py's prioritized case); the priorities of the live rows land on the SAMPLED slots; dead
    rows and undrawn slots keep their priority bit for bit"""
    batch, lr = 160, 0.05
    scale = 16.0 / batch
    fx = nr.fixture(300, 4, 420, seed=11)
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
        rp.set_colour_swap(0.5)
        slots, weights = rp.sample_prioritized(batch)
        d.td_grads_replay(rp, batch, td_net=xq._capi.TD_DOUBLE, mode=0)
        d.apply_grads(lr, scale)
        q_dev, y_dev = d.last_td_values(batch)
        new_w, new_b = d.get_params()
        want = cr.stage(fx, slots, 0.5, 0, RING_SEED)
        assert_staged(d.last_colour_swap(batch), want)
        live = want["action"] >= 0
        assert (~live).any() and want["flags"][live].any() and not want["flags"][live].all()
        S, A, S2, R, D = want["boards"], want["action"], want["next_boards"], fx["R"][slots], fx["D"][slots]
        net, tnet = br.Net(SMALL_NET, w0, b0, br.PRECISION_F32), br.Net(SMALL_NET, wt0, bt0, br.PRECISION_F32)
        f = br.forward(net, S, S2, A, R, D, GAMMA, 2, br.PRECISION_F32, target=tnet)
        _, y_use = br.check_q_y(f, q_dev, y_dev, br.PRECISION_F32)
        u = br.accumulate(net, f, br.backward(net, f, 0, br.PRECISION_F32, weights, y=y_use), br.PRECISION_F32)
        br.check_update(net, u, f, new_w, new_b, lr, scale, br.PRECISION_F32)
        p2 = rp.get_priorities(0, fx["cap"])
        p_dev = (np.abs(q_dev.astype(np.float64) - y_dev) + PER[2]) ** PER[0]
        # a slot drawn by several live rows (some swapped, some not) holds the priority of one of them
        for s in np.unique(slots[live]):
            rows = np.flatnonzero(live & (slots == s))
            assert np.isclose(p2[s], p_dev[rows], rtol=2e-5, atol=0).any(), s
        assert np.abs(br.priorities(f, PER[2], PER[0], y=y_use)[live] ** (1 / PER[0]) - p_dev[live] ** (1 / PER[0])).max() < 2 * br.QTOL
        untouched = np.setdiff1d(np.arange(fx["cap"]), slots[live])
        assert len(np.intersect1d(untouched, slots[~live])) > 0                     # dead rows that were drawn: same bits as before
        assert np.array_equal(p2[untouched].view(np.uint32), prio[untouched].view(np.uint32))
        assert not np.array_equal(p2[slots[live]], prio[slots[live]])
    finally:
        d.close(); rp.close()


# ---- 7. off is off ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", [0.0, 0.5])
def test_prob_zero_is_a_ring_that_was_never_asked(xq, mirror):
    fx = nr.named_fixture("wrapped37")
    never, asked = filled(xq, fx), filled(xq, fx)
    asked.set_colour_swap(0.5)
    asked.set_colour_swap(0.0)
    da, _, _ = make_net(xq, SMALL_NET, seed=4, gamma=GAMMA)
    db, _, _ = make_net(xq, SMALL_NET, seed=4, gamma=GAMMA)
    try:
        for d, rp in ((da, never), (db, asked)):
            if mirror:
                rp.set_mirror(mirror)
            d.kernel_stats(2)
            for _ in range(3):
                rp.sample(65)
                d.td_grads_replay(rp, 65)
                d.apply_grads(0.05, 1.0 / 65)
        sa, sb = da.kernel_stats(), db.kernel_stats()
        assert [(s["name"], s["launches"]) for s in sa] == [(s["name"], s["launches"]) for s in sb]
        names = {s["name"]: s["launches"] for s in sb}
        assert "colour_swap_stage" not in names and "per_writeback" not in names and "nstep_assemble" not in names
        assert names.get("mirror_stage", 0) == (3 if mirror else 0)              # one launch per step, as ever
        (wa, ba), (wb, bb) = da.get_params(), db.get_params()
        assert np.array_equal(wa, wb) and np.array_equal(ba, bb)
        qa, qb = da.last_td_values(65), db.last_td_values(65)
        assert np.array_equal(bits(qa[0]), bits(qb[0])) and np.array_equal(bits(qa[1]), bits(qb[1]))
        if mirror:
            assert_staged(db.last_mirror(65), da.last_mirror(65))
        assert asked.colour_swap() == (0.0, 0)                         # steps taken while prob == 0 do not count
        with pytest.raises(xq.XqError) as e:
            db.last_colour_swap(1)
        assert e.value.code == 2
        # ... and switched on, the bracket is there: one launch per step; the mirror's counter goes its own way
        asked.set_colour_swap(0.5)
        for k in range(2):
            asked.sample(65)
            db.td_grads_replay(asked, 65)
            db.apply_grads(0.0, 1.0)
            st = {s["name"]: s for s in db.kernel_stats()}
            assert st["colour_swap_stage"]["launches"] == k + 1 and st["colour_swap_stage"]["exact"] == k + 1
            assert "nstep_assemble" not in st and "per_writeback" not in st and "legal_side_stage" not in st
        assert asked.colour_swap() == (0.5, 2) and asked.mirror == (mirror, 5 if mirror else 0)
        assert len(db.last_colour_swap(65)["flags"]) == 65
        # raw pointers are never affected: a host-batch step is not a colour-swap-mode one
        db.td_update(fx["S"][:8], fx["S2"][:8], fx["A"][:8], fx["R"][:8], fx["D"][:8], learning_rate=0.0)
        with pytest.raises(xq.XqError) as e:
            db.last_colour_swap(1)
        assert e.value.code == 2
        assert asked.colour_swap() == (0.5, 2)
    finally:
        da.close(); db.close(); never.close(); asked.close()


# ---- 8. trainer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prioritized,overlap,cap,versus", [(0, 0, 64 * 7 + 37, 0), (0, 1, 64 * 7 + 37, 0), (1, 0, 64 * 6 + 19, 0),
                                                           (1, 1, 64 * 6 + 19, 0), (0, 0, 0, 0), (0, 0, 64 * 7 + 37, 1)])
def test_trainer_swaps_its_own_transitions(xq, prioritized, overlap, cap, versus):
    """64 games, 6 iterations, swap 0.5 (cap 0: on-policy, the identity batch; versus: against uniform-random play): every staged row
    is the ring's own transition at the reported slot, transformed iff its flag is set; the flags are the ring's stream; calls advances
    by one per update"""
    G, iters = 64, 6
    mb = 96 if cap else G
    cfg = xq.TrainerConfig(n_games=G, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=GAMMA, epsilon=0.3, replay_capacity=cap,
                           minibatch=mb, td_net=1, target_sync_interval=3, seed=21, prioritized=prioritized, overlap_collect=overlap)
    t = xq.Trainer(cfg)
    try:
        if versus:
            t.set_opponent("random")
        assert t.replay.colour_swap() == (0.0, 0)
        t.set_colour_swap(0.5)
        assert t.replay.colour_swap() == (0.5, 0)
        ring_seed = 21 + 0x1234567
        both = np.zeros(2, bool)
        for it in range(iters):
            if not overlap:
                t.collect()
            t.learn_grads()
            assert t.replay.colour_swap() == (0.5, it + 1) and t.replay.mirror == (0.0, 0)
            with pytest.raises(xq.XqError) as e:
                t.set_colour_swap(0.25)                                # between iterations only
            assert e.value.code == 2
            got = t.dqn.last_colour_swap(mb)
            assert np.array_equal(got["flags"], cr.flags(mb, 0.5, it, ring_seed))
            if not cap:
                assert np.array_equal(got["slot"], np.arange(mb))
            ring = [t.replay.get(int(s)) for s in got["slot"]]
            fx = dict(S=np.array([r[0] for r in ring]), A=np.array([r[1] for r in ring], np.int32), S2=np.array([r[4] for r in ring]))
            want = cr.stage(fx, np.arange(mb), 0.5, it, ring_seed)
            want["slot"] = got["slot"]
            assert_staged(got, want)
            both |= [got["flags"].any(), (got["flags"] == 0).any()]
            moved = got["flags"].astype(bool) & (fx["A"] >= 0)
            assert moved.any() and (got["action"][moved] != fx["A"][moved]).all()      # no square is fixed by row -> 9 - row
            if overlap:
                t.collect()
            t.learn_apply(1)
        assert both.all()
        t.set_colour_swap(0.0)
        if not overlap:
            t.collect()
        t.learn_grads()
        with pytest.raises(xq.XqError):
            t.dqn.last_colour_swap(1)
        if overlap:
            t.collect()
        t.learn_apply(1)
        assert t.replay.colour_swap() == (0.0, iters)
    finally:
        t.close()


# ---- 9. refusals, survival and the facade -------------------------------------------------------------------------------------------
def test_refusals(xq, small):
    rp = xq.ReplayBuffer(40, seed=1)
    try:
        for bad in (float("nan"), -0.1, 1.1, float("inf"), -float("inf")):
            with pytest.raises(xq.XqError) as e:
                rp.set_colour_swap(bad)
            assert e.value.code == 1, bad
        assert rp.colour_swap() == (0.0, 0)
        rp.set_colour_swap(1.0); rp.set_colour_swap(0.0); rp.set_colour_swap(0.5)
        assert rp.colour_swap() == (0.5, 0)
        fresh = xq.DQN(SMALL_NET, 0.01, 0.99, seed=1)
        with pytest.raises(xq.XqError) as e:
            fresh.last_colour_swap(1)
        assert e.value.code == 2
        fresh.close()
    finally:
        rp.close()
    fx = nr.named_fixture("partial37")
    rp = filled(xq, fx)
    try:
        rp.set_colour_swap(0.5)
        rp.sample(8)
        small.td_grads_replay(rp, 8)
        small.apply_grads(0.0, 1.0)
        with pytest.raises(xq.XqError) as e:
            small.last_colour_swap(9)
        assert e.value.code == 1
        with pytest.raises(xq.XqError) as e:
            small.last_colour_swap(8, next_player=True)                # not a step under the legal bootstrap
        assert e.value.code == 1
        assert len(small.last_colour_swap(0)["flags"]) == 0
        assert small.last_colour_swap(8)["boards"].shape == (8, 90)
    finally:
        rp.close()
    t = xq.Trainer(xq.TrainerConfig(n_games=64, layer_sizes=SMALL_NET, minibatch=64, seed=1, replay_capacity=1024))
    try:
        for bad in (float("nan"), -0.1, 1.1):
            with pytest.raises(xq.XqError) as e:
                t.set_colour_swap(bad)
            assert e.value.code == 1, bad
        assert t.replay.colour_swap() == (0.0, 0)
        t.collect()
        t.learn_grads()
        with pytest.raises(xq.XqError) as e:
            t.set_colour_swap(0.5)                                     # a learn_grads waits for its learn_apply
        assert e.value.code == 2
        t.learn_apply(1)
        t.set_colour_swap(0.5)
        assert t.replay.colour_swap() == (0.5, 0)
    finally:
        t.close()


def test_setting_survives_optimizer_params_model_load_target_update_n_step_and_mirror(xq, tmp_path):
    fx = nr.named_fixture("wrapped37")
    rp = filled(xq, fx)
    d, w, b = make_net(xq, SMALL_NET, seed=6, gamma=GAMMA)
    try:
        rp.set_colour_swap(0.5)
        path = str(tmp_path / "m.bin")
        d.saveModel(path)
        changes = (lambda: d.set_optimizer("adam"), lambda: d.set_params(w, b), lambda: d.loadModel(path), lambda: d.updateTargetNetwork(),
                   lambda: rp.set_n_step(2, 4), lambda: rp.set_n_step(1, 4), lambda: rp.set_mirror(0.5), lambda: rp.set_mirror(0.0))
        for call, change in enumerate(changes):
            change()
            assert rp.colour_swap() == (0.5, call)
            slots = rp.sample(65)
            d.td_grads_replay(rp, 65)
            d.apply_grads(0.01, 1.0 / 65)
            got = d.last_colour_swap(65)
            if rp.n_step[0] == 1 and rp.mirror[0] == 0.0:
                assert_staged(got, cr.stage(fx, slots, 0.5, call, RING_SEED))
            else:
                assert np.array_equal(got["flags"], cr.flags(65, 0.5, call, RING_SEED)) and np.array_equal(got["slot"], slots)
        assert rp.mirror == (0.0, 1)
    finally:
        d.close(); rp.close()


def test_facade_carries_colour_swap_onto_the_trainers_ring(xq):
    from test_colour_swap_ref_cpu import build_colour_swap_facade_probe
    exe = build_colour_swap_facade_probe()
    out = subprocess.run([exe, "64", "40", "7", "0.5"], check=True, capture_output=True, text=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["ring_before"], r["ring_after"], r["ring_mirror"]) == (0.0, 0.5, 0.0)
    assert r["big_refused"] == 1 and r["nan_refused"] == 1 and r["ai_neg_refused"] == 1 and r["ai_nan_refused"] == 1
    assert (r["ai_before"], r["ai_after"]) == (0.0, 0.5)
    assert r["plain_swap"] == 0.0 and r["swapped_swap"] == 0.5 and r["stats_mirror"] == 0.0
    assert r["plain_updates"] > 0 and r["swapped_updates"] > 0
    assert r["plain_finite"] == 1 and r["swapped_finite"] == 1
