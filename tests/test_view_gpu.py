"""The mover view (xq_dqn_set_view, DESIGN.md §4 "Mover view") on the device — `pytest -m gpu`: view_boards_kernel against numpy on
every nibble; the env's pick through the view's square map; the ring's who-moved column; the batch mover_view_stage_kernel stages against
tests/view_ref.py on every nibble (gather form, behind the n-step assembly, behind the mirror, behind both, under the legal bootstrap);
the step bit for bit against the existing step on the host-built batch; absolute again is a handle that was never asked; the refusals;
the arena."""
import os

import numpy as np
import pytest

import colour_swap_ref as cr
import mirror_ref as mr
import nstep_ref as nr
import view_ref as vr
from first_max import pick
from test_legal_gpu import legal_net, pool, rows_of

pytestmark = pytest.mark.gpu

SMALL_NET = [1260, 64, 64, 8100]
GAMMA = 0.97
RING_SEED = 5
CAP, STRIDE = 256, 4
PER = (0.6, 0.4, 1e-3)


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


@pytest.fixture(scope="module")
def sparse(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_sparse.npz"))["board"].astype(np.uint8)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def make_net(xq, sizes=SMALL_NET, seed=8, gamma=GAMMA, legal=False):
    if legal:
        d = legal_net(xq, sizes, seed)
        if gamma != GAMMA:
            d2 = xq.DQN(sizes, 0.001, gamma, seed=seed)
            d2.set_params(*d.get_params()); d2.set_params(*d.get_params(1), net=1); d2.set_td_bootstrap("legal")
            d.close()
            return d2
        return d
    from test_dqn_gpu import make_net as mk
    d, _, _ = mk(xq, sizes, seed=seed, gamma=gamma)
    wt, bt = d.get_params()
    rng = np.random.default_rng(seed + 1)
    d.set_params(wt + rng.uniform(-0.01, 0.01, wt.shape), bt + rng.uniform(-0.01, 0.01, bt.shape), net=1)     # a target net of its own
    return d


_ring = {}


def ring_fixture(golden_dir):
    """256 transitions of tests/test_legal_gpu.py's pool (ref_bigmoves and ref_sparse rows, sides without a move, done and dead rows)
    with the side to move in s' the pool's and the mover drawn per row: half the rows self-play rows (mover = 1 - next side), half versus
    rows (mover = next side).  Built once, never written."""
    if not _ring:
        b = rows_of(pool(golden_dir), np.concatenate([np.arange(128), 320 + np.arange(128)]))
        rng = np.random.default_rng(9)
        selfplay = rng.random(CAP) < 0.5
        mover = np.where(selfplay, 1 - b["side"], b["side"]).astype(np.uint8)
        _ring.update(S=b["S"], A=b["A"], R=b["R"], D=b["D"], S2=b["S2"], mover=mover, next_player=b["side"].astype(np.uint8), cap=CAP,
                     stride=STRIDE)
        assert set(np.unique(mover)) == {0, 1} and set(np.unique(b["side"])) == {0, 1} and (mover != b["side"]).any() and (mover == b["side"]).any()
        assert (b["A"] < 0).any() and b["D"].any()
    return _ring


def filled(xq, fx, per=None, track=(True, True)):
    rp = xq.ReplayBuffer(fx["cap"], seed=RING_SEED)
    if per:
        rp.enable_per(*per)
    if track[0]:
        rp.track_mover()
    if track[1]:
        rp.track_next_player()
    rp.push(fx["S"], fx["A"], fx["R"], fx["D"], fx["S2"], mover=fx["mover"] if track[0] else None,
            next_player=fx["next_player"] if track[1] else None)
    return rp


def assert_staged(got, want):
    for k in ("flag_s", "flag_next", "boards", "next_boards", "action", "slot"):
        assert np.array_equal(got[k], want[k]), k


def same_step(a, b, batch):
    (qa, ya), (qb, yb) = a.last_td_values(batch), b.last_td_values(batch)
    assert np.array_equal(bits(qa), bits(qb)) and np.array_equal(bits(ya), bits(yb))
    assert a.last_loss() == b.last_loss()
    for net in (0, 1):
        (wa, ba), (wb, bb) = a.get_params(net), b.get_params(net)
        assert np.array_equal(wa, wb) and np.array_equal(ba, bb)


# ---- 1. view_boards_kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_view_boards_equals_numpy_on_every_nibble(xq, sparse, n):
    from cn_chess_ai_amd.dqn import view_boards_packed
    red = ((sparse >= 1) & (sparse <= 7)).sum(axis=1)
    black = (sparse >= 8).sum(axis=1)
    bare = np.flatnonzero((red == 0) | (black == 0))
    assert len(bare) > 0                                           # boards on which one side has no piece at all
    order = np.concatenate([bare, np.setdiff1d(np.arange(len(sparse)), bare)])
    B = np.concatenate([sparse[order], xq.START_BOARD.reshape(1, 90).astype(np.uint8)])[np.arange(n) % (len(sparse) + 1)]
    if n >= 63:                                                    # every code on every square, 15 squares at a time
        for k in range(1, 15):
            B[k + 1] = 0
            B[k + 1, (15 * (k % 6)):(15 * (k % 6)) + 15] = k
    words = np.array([cr.pack(b) for b in B], np.uint32)
    rng = np.random.default_rng(n)
    for sides in (np.zeros(n, np.uint8), np.ones(n, np.uint8), rng.integers(0, 2, n).astype(np.uint8), (rng.integers(0, 2, n) * 255).astype(np.uint8)):
        want = vr.view(B, sides)
        got = xq.view_boards(B, sides)
        assert got.shape == (n, 90) and np.array_equal(got, want)
        out = view_boards_packed(words, sides)
        assert np.array_equal(out, np.array([cr.pack(b) for b in want], np.uint32))       # the words: nibbles 90..95 stay 0
        assert not (out[:, 11] >> 8).any()
    assert np.array_equal(xq.view_boards(B, np.zeros(n, np.uint8)), B)


# ---- 2. the pick --------------------------------------------------------------------------------------------------------------------
def test_pick_reads_black_rows_through_the_square_map(xq, sparse):
    import xqoracle as xo
    n, seed = 5, 77
    usable = []
    for b in sparse:                                               # both generals on the board and both sides with a move
        if (b == 1).sum() == 1 and (b == 8).sum() == 1 and all(xo.all_valid_actions(xo.board_from(b, player=c), c)[1] > 1 for c in (0, 1)):
            usable.append(b)
        if len(usable) == 3:
            break
    boards = np.stack([xq.START_BOARD.reshape(90).astype(np.uint8), usable[0], usable[1], usable[2], xq.START_BOARD.reshape(90).astype(np.uint8)])
    side = np.array([0, 1, 0, 1, 1], np.int32)
    q = ((np.random.default_rng(1).permutation(n * 90).reshape(n, 90) + 0.5) / (n * 90) * 1.8 - 0.9).astype(np.float32)
    assert len(np.unique(q)) == n * 90                             # pairwise distinct: no tie anywhere
    envs = [xq.VecEnv(n, seed=seed) for _ in range(3)]
    try:
        states = []
        for e in envs:
            _, meta = e.get_state()
            meta[:, 0] = side                                      # one ply played where Black is to move
            meta[:, 1] = side
            e.set_state(boards, meta)
            states.append(e.get_state())
        A, B, Cn = envs
        B.set_q_view(True); Cn.set_q_view(True)
        assert B.q_view and not A.q_view
        ra = A.selfplay_step(q, 0.0)
        rb = B.selfplay_step(vr.pick_rows(q, side), 0.0)
        rc = Cn.selfplay_step(q, 0.0)                               # control: the view's map on rows that are not in the view
        assert np.array_equal(ra, rb)
        (ba, ma), (bb, mb) = A.get_state(), B.get_state()
        assert np.array_equal(ba, bb) and np.array_equal(ma, mb) and not np.array_equal(ba, boards)
        assert not ra["explored"].any() and ra["valid"].all()
        red = side == 0
        assert np.array_equal(ra[red], rc[red]) and (ra["action"][~red] != rc["action"][~red]).any()
        # the move itself, from the lists: the first maximum over q[to]
        for g in range(n):
            codes, cnt = xo.all_valid_actions(xo.board_from(boards[g], player=int(side[g])), int(side[g]))
            assert int(ra["action"][g]) == int(codes[pick(q[g], codes[:cnt])])
    finally:
        for e in envs:
            e.close()


# ---- 3. the ring's columns ----------------------------------------------------------------------------------------------------------
def test_selfplay_ring_records_who_moved(xq):
    n, plies = 48, 8
    env = xq.VecEnv(n, seed=21)
    rp = xq.ReplayBuffer(n * plies, seed=4)
    try:
        rp.track_mover(); rp.track_mover()                          # a second call is a no-op
        rp.track_next_player()
        boards0, meta0 = env.get_state()
        meta0[: n // 3, 0] = 200 - 1 - np.arange(n // 3) % 5          # games near the 200-ply cap: terminal plies and resets inside the run
        meta0[: n // 3, 1] = meta0[: n // 3, 0] & 1
        env.set_state(boards0, meta0)
        want = np.zeros((plies, n), np.uint8)
        for it in range(plies):
            want[it] = env.get_state()[1][:, 1]
            env.selfplay_step_dev(0, 96, 1.0, replay=rp)
        env.get_state(0, 1)
        assert set(np.unique(want)) == {0, 1}
        assert np.array_equal(rp.mover(0, n * plies).reshape(plies, n), want)
        assert np.array_equal(rp.next_player(0, n * plies).reshape(plies, n), 1 - want)
        for push in (lambda: rp.push(boards0[:1], [3], [0.0], [0], boards0[:1]),
                     lambda: rp.push(boards0[:1], [3], [0.0], [0], boards0[:1], next_player=[1])):
            with pytest.raises(xq._capi.XqError) as e:
                push()
            assert e.value.code == 1 and "push_host_sides" in str(e.value)
        with pytest.raises(xq._capi.XqError) as e:
            rp.push(boards0[:1], [3], [0.0], [0], boards0[:1], mover=[2], next_player=[1])
        assert e.value.code == 1
        rp.push(boards0[:2], [3, 4], [0.0, 0.5], [0, 1], boards0[:2], mover=[1, 0], next_player=[0, 0])
        assert rp.mover(0, 2).tolist() == [1, 0] and rp.next_player(0, 2).tolist() == [0, 0]
    finally:
        env.close(); rp.close()


def test_versus_ring_records_the_learners_colour_and_tracking_needs_an_empty_ring(xq):
    n, first = 32, 3
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=GAMMA, epsilon=0.2, replay_capacity=n * 8,
                           minibatch=n, td_net=0, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=9,
                           first_game_id=first, collects_per_update=1, overlap_collect=0)
    t = xq.Trainer(cfg)
    rp = xq.ReplayBuffer(8, seed=1)
    try:
        t.set_opponent("random")
        t.set_view("mover")
        assert t.dqn.view() == "mover" and t.env.q_view
        t.step(5)
        colour = np.tile((first + np.arange(n)) & 1, (5, 1))
        assert np.array_equal(t.replay.mover(0, n * 5).reshape(5, n), colour)
        assert np.array_equal(t.replay.next_player(0, n * 5).reshape(5, n), colour)
        w, b = t.dqn.get_params()
        assert np.isfinite(w).all() and np.isfinite(b).all()
        f = t.dqn.last_view(n)
        assert np.array_equal(f["flag_s"], f["flag_next"]) and set(np.unique(f["flag_s"])) == {0, 1}
        # an untracked ring has no column; a ring that holds a transition cannot start tracking
        b1 = np.zeros((1, 90), np.uint8); b1[0, 4], b1[0, 85] = 1, 8
        with pytest.raises(xq._capi.XqError) as e:
            rp.mover(0, 1)
        assert e.value.code == 2
        with pytest.raises(xq._capi.XqError) as e:
            rp.push(b1, [3], [0.0], [0], b1, mover=[0])
        assert e.value.code == 1 and "track_mover" in str(e.value)
        rp.push(b1, [3], [0.0], [0], b1)
        with pytest.raises(xq._capi.XqError) as e:
            rp.track_mover()
        assert e.value.code == 2 and "already holds" in str(e.value)
    finally:
        t.close(); rp.close()


# ---- 4. the staged batch ------------------------------------------------------------------------------------------------------------
def staged_reference(fx, slots, n_step, mirror, call):
    """(want, R, D) of a view-mode step: n-step assembly, then the mirror, then the view — the flags from the ring's columns at the
    assembly's first and last slot"""
    first = last = np.asarray(slots, np.int32)
    S, A, R, D, S2 = fx["S"][slots], fx["A"][slots], fx["R"][slots], fx["D"][slots], fx["S2"][slots]
    ref = None
    if n_step > 1:
        ref = nr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n_step, fx["stride"], GAMMA, 0, fx["cap"])
        S, A, R, D, S2 = nr.staged(fx, ref)
        first, last = ref["first_slot"], ref["last_slot"]
    if mirror > 0:
        m = mr.apply(S, A, S2, mirror, call, RING_SEED)
        S, A, S2 = m["boards"], m["action"], m["next_boards"]
    want = vr.apply(S, A, S2, fx["mover"][first], fx["next_player"][last])
    want["slot"] = np.asarray(slots, np.int32)
    return want, R, D, ref


@pytest.mark.parametrize("n_step,mirror", [(1, 0.0), (3, 0.0), (1, 1.0), (1, 0.5), (3, 0.5)])
def test_staged_batch_equals_the_reference_on_every_nibble(xq, golden_dir, n_step, mirror):
    fx = ring_fixture(golden_dir)
    rp = filled(xq, fx)
    d = make_net(xq)
    try:
        d.set_view("mover")
        if n_step > 1:
            rp.set_n_step(n_step, fx["stride"])
        if mirror:
            rp.set_mirror(mirror)
        for call, batch in enumerate((1, 63, 64, 65, 0)):
            slots = rp.sample(batch) if batch else np.arange(fx["cap"], dtype=np.int32)
            rows = len(slots)
            d.kernel_stats(2)
            d.td_grads_replay(rp, batch)
            d.apply_grads(0.0, 1.0)
            st = {s["name"]: s["launches"] for s in d.kernel_stats()}
            d.kernel_stats(0)
            assert st["mover_view_stage"] == 1 and ("nstep_assemble" in st) == (n_step > 1) and ("mirror_stage" in st) == (mirror > 0)
            assert "colour_swap_stage" not in st and "legal_side_stage" not in st
            want, _, _, ref = staged_reference(fx, slots, n_step, mirror, call)
            got = d.last_view(rows)
            assert_staged(got, want)
            if rows >= 63:
                both = got["flag_s"] != got["flag_next"]
                assert both.any() and (~both).any()                 # rows whose two boards take different masks, and rows where they agree
                assert (got["action"] != (ref["action"] if ref else fx["A"][slots]))[got["flag_s"] == 1].any() or mirror > 0
            if ref is not None:
                ns = d.last_n_step(rows)
                assert np.array_equal(ns["first_slot"], ref["first_slot"]) and np.array_equal(ns["last_slot"], ref["last_slot"])
                if rows >= 63:
                    assert (ref["steps"] < n_step).any() and (ref["steps"] == n_step).any() and ref["dead"].any()      # rows cut short
                    assert (ref["last_slot"] != ref["first_slot"]).any()
            if mirror:
                assert np.array_equal(d.last_mirror(rows)["flags"], mr.flags(rows, mirror, call, RING_SEED))       # a reflection changes no side
        # the ring was never written
        for s in (0, 17, fx["cap"] - 1):
            b, a, r, dn, nb = rp.get(s)
            assert np.array_equal(b, fx["S"][s]) and np.array_equal(nb, fx["S2"][s]) and a == fx["A"][s]
        assert np.array_equal(rp.mover(), fx["mover"]) and np.array_equal(rp.next_player(), fx["next_player"])
    finally:
        d.close(); rp.close()


# ---- 5. the step is the existing step on the host-built batch -----------------------------------------------------------------------
@pytest.mark.parametrize("opt,loss,zero_sum,td_net,legal,n_step,mirror", [
    ("sgd", "squared", False, 0, False, 1, 0.0),
    ("adam", "huber", True, 2, False, 1, 0.5),
    ("sgd", "huber", True, 2, True, 1, 0.0),
    ("adam", "squared", False, 1, True, 1, 0.5),
    ("sgd", "squared", False, 2, True, 3, 0.0),
    ("adam", "huber", False, 0, False, 3, 0.5),
])
def test_step_is_the_existing_step_on_the_view_batch(xq, golden_dir, opt, loss, zero_sum, td_net, legal, n_step, mirror):
    batch, lr = 65, 0.05
    fx = ring_fixture(golden_dir)
    rp = filled(xq, fx)
    disc = nr.discounts(GAMMA, n_step)
    a = make_net(xq, legal=legal)
    b = make_net(xq, legal=legal, gamma=float(disc[n_step]) if n_step > 1 else GAMMA)
    try:
        w0, _ = a.get_params()
        for d in (a, b):
            d.set_optimizer(opt)
            d.set_td_loss(loss, 0.05)
            d.set_zero_sum(zero_sum)
        a.set_view("mover")
        if n_step > 1:
            rp.set_n_step(n_step, fx["stride"])
        if mirror:
            rp.set_mirror(mirror)
        slots = rp.sample(batch)
        a.kernel_stats(2)
        a.td_grads_replay(rp, batch, td_net=td_net)
        a.apply_grads(lr, 1.0 / batch)
        st = {s["name"]: s["launches"] for s in a.kernel_stats()}
        a.kernel_stats(0)
        assert st["mover_view_stage"] == 1 and "legal_side_stage" not in st and ("legal_qmax" in st) == legal
        want, R, D, _ = staged_reference(fx, slots, n_step, mirror, 0)
        assert_staged(a.last_view(batch), want)
        # the existing entry point on view_ref's batch; under `legal` the sided one with Red to move on every row
        b.td_update(want["boards"], want["next_boards"], want["action"], R, D, td_net=td_net, learning_rate=lr, grad_scale=1.0 / batch,
                    next_player=want["next_player"] if legal else None)
        same_step(a, b, batch)
        assert np.abs(a.get_params()[0] - w0).max() > 0
        if legal:
            La, Lb = a.last_legal(batch, z96=False), b.last_legal(batch, z96=False)
            for k in ("n_moves", "a_star"):
                assert np.array_equal(La[k], Lb[k]), k
            assert np.array_equal(bits(La["zmax"]), bits(Lb["zmax"])) and (La["n_moves"] > 0).any()
            # control: with the ring's absolute side bytes instead of 0 the view boards have other moves
            ctl = make_net(xq, legal=True, gamma=float(disc[n_step]) if n_step > 1 else GAMMA)
            try:
                side = fx["next_player"][a.last_n_step(batch)["last_slot"] if n_step > 1 else slots]
                ctl.td_update(want["boards"], want["next_boards"], want["action"], R, D, td_net=td_net, learning_rate=0.0, next_player=side)
                assert not np.array_equal(ctl.last_legal(batch, z96=False)["n_moves"], La["n_moves"])
            finally:
                ctl.close()
    finally:
        a.close(); b.close(); rp.close()


def test_prioritized_view_step_writes_its_priorities_to_the_sampled_slots(xq, golden_dir):
    batch = 160
    fx = ring_fixture(golden_dir)
    rp = filled(xq, fx, per=PER)
    a, b = make_net(xq), make_net(xq)
    try:
        a.set_view("mover")
        prio = np.random.default_rng(5).uniform(1.0, 2.0, size=fx["cap"]).astype(np.float32)
        rp.set_priorities(prio)
        rp.per_rebuild()
        slots, _ = rp.sample_prioritized(batch)
        before = rp.get_priorities(0, fx["cap"])
        a.td_grads_replay(rp, batch, td_net=2)
        a.apply_grads(0.0, 1.0)
        want, R, D, _ = staged_reference(fx, slots, 1, 0.0, 0)
        assert_staged(a.last_view(batch), want)
        qa, ya = a.last_td_values(batch)
        # the host step has no importance weights: targets and Q(s, a) agree bit for bit, and the priorities follow them
        qb, yb = b.td_update(want["boards"], want["next_boards"], want["action"], R, D, td_net=2, learning_rate=0.0)
        assert np.array_equal(bits(qa), bits(qb)) and np.array_equal(bits(ya), bits(yb))
        after = rp.get_priorities(0, fx["cap"])
        live = want["action"] >= 0
        expect = (np.abs(qa.astype(np.float64) - ya) + PER[2]) ** PER[0]
        for s in set(int(x) for x in slots[live]):
            dup = [j for j in range(batch) if slots[j] == s and live[j]]
            assert min(abs(after[s] / expect[j] - 1) for j in dup) < 2e-5        # (fp32 powf against fp64: test_legal_ring_gpu's bound)
        rest = np.setdiff1d(np.arange(fx["cap"]), slots[live])
        assert np.array_equal(after[rest], before[rest]) and live.any() and (~live).any()
    finally:
        a.close(); b.close(); rp.close()


# ---- 6. absolute again ----------------------------------------------------------------------------------------------------------------
def test_absolute_after_mover_is_a_handle_that_was_never_asked(xq, golden_dir):
    batch, lr = 65, 0.05
    fx = ring_fixture(golden_dir)
    rp, rq = filled(xq, fx), filled(xq, fx)
    a, b = make_net(xq), make_net(xq)
    try:
        assert a.view() == "absolute"
        a.set_view("mover")
        a.td_grads_replay(rp, 0)
        a.apply_grads(0.0, 1.0)                                    # (SGD at rate 0: the parameters stand)
        a.set_view("absolute")
        assert a.view() == "absolute"
        for rule, mirror in ((0, 0.0), (2, 0.5)):
            for ring in (rp, rq):
                ring.set_mirror(mirror)
            outs = []
            for d, ring in ((a, rp), (b, rq)):
                slots = ring.sample(batch)
                d.kernel_stats(2)
                d.td_grads_replay(ring, batch, td_net=rule)
                d.apply_grads(lr, 1.0 / batch)
                outs.append((slots, [(s["name"], s["launches"]) for s in d.kernel_stats()]))
                d.kernel_stats(0)
                with pytest.raises(xq.XqError):
                    d.last_view(1)
            if mirror == 0.0:
                assert np.array_equal(outs[0][0], outs[1][0])
            assert outs[0][1] == outs[1][1] and not any("view" in n for n, _ in outs[0][1])
            if mirror == 0.0:
                same_step(a, b, batch)
    finally:
        a.close(); b.close(); rp.close(); rq.close()


# ---- 7. refusals and survival -----------------------------------------------------------------------------------------------------------
def test_refusals(xq, golden_dir, tmp_path):
    fx = ring_fixture(golden_dir)
    rp = filled(xq, fx)
    only_next, neither = filled(xq, fx, track=(False, True)), filled(xq, fx, track=(False, False))
    d = make_net(xq)
    try:
        with pytest.raises(ValueError):
            d.set_view("sideways")
        with pytest.raises(xq.XqError) as e:
            xq._capi.call("xq_dqn_set_view", d.handle, 2)
        assert e.value.code == 1
        d.set_view("mover")
        # survives every other setter, new parameters, a model load and a target update
        w, b = d.get_params()
        d.set_optimizer("adam"); d.set_params(w, b); d.updateTargetNetwork(); d.set_precision(xq._capi.PRECISION_F32)
        d.set_td_loss("huber", 0.1); d.set_zero_sum(True); d.set_zero_sum(False); d.set_td_bootstrap("all")
        path = str(tmp_path / "m.bin")
        size_before = None
        d.saveModel(path)
        size_before = os.path.getsize(path)
        d.set_view("absolute"); d.saveModel(path)
        assert os.path.getsize(path) == size_before                # the model file does not carry the view
        d.set_view("mover"); d.loadModel(path)
        assert d.view() == "mover"
        d.set_optimizer("sgd")
        # colour swap together with the view: the message names both setters
        rp.set_colour_swap(0.5)
        with pytest.raises(xq.XqError) as e:
            d.td_grads_replay(rp, 0)
        assert e.value.code == 1 and "xq_dqn_set_view" in str(e.value) and "xq_replay_set_colour_swap" in str(e.value)
        rp.set_colour_swap(0.0)
        # a ring that does not track both columns
        for ring in (only_next, neither):
            with pytest.raises(xq.XqError) as e:
                d.td_grads_replay(ring, 0)
            assert e.value.code == 1 and "xq_replay_track_mover" in str(e.value)
        with pytest.raises(xq.XqError):
            d.last_view(1)
        # the setter while an apply is pending (a fused apply keeps the step's slab sums for it: 1024 rows, as its siblings' tests)
        big = dict(fx, cap=4 * fx["cap"], **{k: np.tile(fx[k], (4, 1) if fx[k].ndim == 2 else 4) for k in ("S", "A", "R", "D", "S2", "mover", "next_player")})
        rb = filled(xq, big)
        from test_dqn_gpu import REF_NET
        dz = make_net(xq, REF_NET)
        try:
            dz.set_view("mover")
            dz.set_fused_apply(True)
            dz.td_grads_replay(rb, 0)
            with pytest.raises(xq.XqError) as e:
                dz.set_view("absolute")
            assert e.value.code == 2 and "waiting" in str(e.value) and dz.view() == "mover"
            dz.apply_grads(0.0, 1.0)
            dz.set_view("absolute")
        finally:
            rb.close(); dz.close()
        d.td_grads_replay(rp, 0)
        d.apply_grads(0.0, 1.0)
        with pytest.raises(xq.XqError) as e:
            d.last_view(fx["cap"] + 1)
        assert e.value.code == 1
        d.set_view("absolute")
        # DQN.train reads absolute boards on the host
        d.set_view("mover")
        with pytest.raises(ValueError):
            d.train(np.zeros(1260), 3, 0.0, np.zeros(1260), False)
    finally:
        d.close(); rp.close(); only_next.close(); neither.close()


def test_trainer_set_view_after_a_collect_is_refused(xq):
    cfg = xq.TrainerConfig(n_games=32, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=0.99, epsilon=0.2, replay_capacity=128,
                           minibatch=32, td_net=0, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=3,
                           first_game_id=0, collects_per_update=1, overlap_collect=0)
    t = xq.Trainer(cfg)
    try:
        with pytest.raises(ValueError):
            t.set_view("some")
        t.collect()
        with pytest.raises(xq.XqError) as e:
            t.set_view("mover")
        assert e.value.code == 2 and t.dqn.view() == "absolute" and not t.env.q_view
        t.learn_grads(); t.learn_apply()
        t.step(2)                                                  # the absolute view goes on
    finally:
        t.close()


# ---- 8. the arena -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opening", [2, 3])
def test_arena_reads_a_view_net_through_the_square_map(xq, opening):
    """one ply past the opening, 3 pairs, a view net (A) against random play: with an even opening Red is to move and A moves in the half
    where it is Red, with an odd one Black is and A moves in the half where it is Black — there the pick is taken at swap(to)"""
    pairs = 3
    arena = xq.Arena(pairs, seed=11, opening_plies=opening)
    probe = xq.VecEnv(2 * pairs, seed=1)
    d = make_net(xq)
    try:
        d.set_view("mover")
        assert arena.run(d, None, max_plies=opening) == opening
        boards, meta = arena.env.get_state()
        side = meta[:, 1]
        assert (side == opening % 2).all()
        codes, counts = arena.env.legal_moves()
        probe.set_state(vr.view(boards, side))                      # the host-built view boards, through xq_dqn_forward_boards_dev
        q = d.q_boards(probe, 96).cpu().numpy()
        assert arena.run(d, None, max_plies=1) == 1
        res = arena.last_step()
        moved = 0
        for g in range(2 * pairs):
            a_is_red = g < pairs
            if a_is_red != (opening % 2 == 0) or counts[g] == 0:
                continue                                           # the random player's half
            row = q[g, :90]
            if side[g]:
                row = row[cr.swap_action(np.arange(90))]           # row[t] = q[swap(t)]
            assert int(res["action"][g]) == int(codes[g][pick(row, codes[g][:counts[g]])]) and not res["explored"][g]
            moved += 1
        assert moved == pairs
        # control: the same ply read without the map is another move somewhere on the Black half
        if opening % 2 == 1:
            plain = [int(codes[g][pick(q[g, :90], codes[g][:counts[g]])]) for g in range(pairs, 2 * pairs)]
            assert plain != [int(x) for x in res["action"][pairs:]]
    finally:
        arena.close(); probe.close(); d.close()


def test_arena_ply_with_caller_rows_in_the_view_is_the_run_players_ply(xq):
    """xq_arena_ply_q_dev_view with rows the caller computed on view_boards' boards plays the ply xq_arena_run plays for a view net (the
    other player explores always, which is the random player's draw), and without the flag it does not"""
    import torch
    pairs, opening = 3, 3
    arenas = [xq.Arena(pairs, seed=11, opening_plies=opening) for _ in range(3)]
    probe = xq.VecEnv(2 * pairs, seed=1)
    d = make_net(xq)
    try:
        d.set_view("mover")
        for a in arenas:
            assert a.run(d, None, max_plies=opening) == opening
        boards, meta = arenas[0].env.get_state()
        probe.set_state(xq.view_boards(boards, meta[:, 1]))
        q = d.q_boards(probe, 96)
        arenas[0].run(d, None, max_plies=1)
        arenas[1].ply_q_dev(q, eps_a=0.0, eps_b=1.0, view_a=True)
        arenas[2].ply_q_dev(q, eps_a=0.0, eps_b=1.0)
        torch.cuda.synchronize()
        want, got, plain = (a.last_step() for a in arenas)
        assert np.array_equal(want["action"], got["action"]) and np.array_equal(arenas[0].env.get_state()[0], arenas[1].env.get_state()[0])
        assert not np.array_equal(want["action"][pairs:], plain["action"][pairs:])          # A moves as Black in the second half
        assert np.array_equal(want["action"][:pairs], plain["action"][:pairs])
    finally:
        for a in arenas:
            a.close()
        probe.close(); d.close()


def test_versus_net_opponent_is_read_through_its_own_view(xq):
    """the opponent's handle carries its view: the same frozen net as opponent, once with the absolute and once with the mover view, plays
    other games against the same learner"""
    n = 32
    outs = []
    for view in ("absolute", "mover"):
        cfg = xq.TrainerConfig(n_games=n, layer_sizes=SMALL_NET, learning_rate=0.01, gamma=GAMMA, epsilon=0.0, replay_capacity=n * 8,
                               minibatch=n, td_net=0, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=9,
                               first_game_id=0, collects_per_update=1, overlap_collect=1)
        t = xq.Trainer(cfg)
        opp = make_net(xq, seed=21)
        try:
            opp.set_view(view)
            w_opp = opp.get_params()[0].copy()
            t.set_view("mover")
            t.set_opponent((opp, 0.0))
            t.step(6)
            boards, meta = t.env.get_state()
            w, b = t.dqn.get_params()
            assert np.isfinite(w).all() and np.isfinite(b).all()
            assert np.array_equal(opp.get_params()[0], w_opp) and opp.view() == view      # a lent net keeps its bits and its view
            outs.append(boards)
        finally:
            t.close(); opp.close()
    assert not np.array_equal(outs[0], outs[1])
