"""The zero-sum TD target (xq_dqn_set_zero_sum, DESIGN.md §4 "Zero-sum target") on the device — `pytest -m gpu`.

1. One small step per kernel body that forms a target (tests/td_edge_cases.py's families), each checked three ways: (a) Q(s,a), y, the
   loss and every parameter against tests/zero_sum_ref.py with batch_ref's tolerances; (b) with all rewards 0, y is minus the y of a twin
   handle without zero-sum, bit for bit; (c) set_zero_sum(False) after True is a handle that was never asked.
2. Prioritized replay: the written-back priorities follow the new y.
3. The legal-move bootstrap: a side without a move is worth -1 (zmax = -inf, y = fl32(r + g)), every other row is selected as before.
4. n-step batches: the assembled rewards are zero_sum_ref's bit for bit and the step is the 1-step step on the assembled batch with the
   discount disc_n; alone, behind the mirror, behind the colour swap, under the legal bootstrap, uniform and prioritized.
5. The setters: arguments, the pending-apply refusal, and what the setting survives.
"""
import numpy as np
import pytest

import batch_ref as br
import huber_ref as hr
import legal_ref as lr
import nstep_ref as nr
import td_edge_cases as tc
import zero_sum_ref as zr
from test_dqn_gpu import CFG2_NET, make_net
from test_td_shape_edges_gpu import batch_of, net_of

pytestmark = pytest.mark.gpu

SMALL_NET = [1260, 64, 64, 8100]
GAMMA = 0.99                                    # (what test_td_shape_edges_gpu.net_of's handles carry)
NGAMMA = 0.97                                   # the ring tests' discount
KAPPA = 0.05
PER = (0.6, 0.4, 1e-3)
RING_SEED = 5


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. one step per body ----------------------------------------------------------------------------------------------------------------
A256, A512, F64 = "1260-256-256-8100", "1260-512-512-8100", "1260-64-64-8100"
# name: (net, n, rule, precision, huber, screened path expected, TD delta inside the refine kernel)
STEPS = {
    "f32_256_body": (A256, 300, 0, 0, False, False, False),
    "f32_512_body": (A512, 300, 0, 0, False, False, False),
    "bf16_512_body_double_p1": (A512, 300, 2, 1, False, False, False),
    "bf16_512_body_double_p2": (A512, 300, 2, 2, False, False, False),
    "general_body_64": (F64, 65, 0, 0, False, False, False),
    "general_body_256_double": (A256, 300, 2, 0, False, False, False),
    "refine_64": (F64, 1024, 0, 0, False, True, False),
    "refine_256_delta_inside": (A256, 1024, 0, 0, False, True, True),
    "huber_f32_256_body": (A256, 300, 0, 0, True, False, False),
    "huber_refine_256_delta_inside": (A256, 1024, 0, 0, True, True, True),
    "huber_bf16_512_body_double": (A512, 300, 2, 1, True, False, False),
}


def case_of(name):
    net, n, rule, prec, huber, screened, inside = STEPS[name]
    return tc._case("z", net, n, rule, prec), huber, screened, inside


def handle_of(xq, c, huber, zero_sum):
    d = net_of(xq, c)
    d.set_precision(c.prec)
    if huber:
        d.set_td_loss("huber", KAPPA)
    if zero_sum is not None:
        d.set_zero_sum(zero_sum)
    return d


def step(d, c, batch, R=None, lr=None):
    S, A, Rb, D, S2 = batch
    return d.td_update(S, S2, A, Rb if R is None else R, D, td_net=c.rule, mode=c.mode, learning_rate=c.lr if lr is None else lr,
                       grad_scale=c.scale)


@pytest.mark.parametrize("name", list(STEPS))
def test_step_matches_the_written_out_rule(xq, name):
    """(a): Q(s,a), y, the loss and the updated parameters against zero_sum_ref, tolerances of batch_ref.check_q_y and check_update"""
    c, huber, screened, inside = case_of(name)
    batch = batch_of(xq, c.n, c.seed)
    S, A, R, D, S2 = batch
    d = handle_of(xq, c, huber, True)
    try:
        assert d.zero_sum() is True
        w0, b0 = d.get_params()
        wt0, bt0 = d.get_params(1)
        d.kernel_stats(2)
        q_dev, y_dev = step(d, c, batch)
        launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
        loss_dev = d.last_loss()
        new_w, new_b = d.get_params()
        net = br.Net(c.sizes, w0, b0, c.prec)
        tnet = br.Net(c.sizes, wt0, bt0, c.prec) if c.rule != 0 else None
        f = zr.forward(net, S, S2, A, R, D, GAMMA, c.rule, c.prec, target_net=tnet)
        flipped, y_use = br.check_q_y(f, q_dev, y_dev, c.prec)
        loss_ref = hr.loss(f, KAPPA, y=y_use) if huber else br.loss(f, y_use)
        print("loss", loss_dev, loss_ref, "flipped", len(flipped), "launches", launches)
        assert abs(loss_dev - loss_ref) <= br.LOSS_RTOL[c.prec] * loss_ref, (loss_dev, loss_ref)
        weights = hr.weights(f, KAPPA, None, y=y_use) if huber else None
        bk = br.backward(net, f, c.mode, c.prec, weights, y=y_use, bf16_layers=tc.bf16_delta_layers(c))
        u = br.accumulate(net, f, bk, c.prec, bf16_layers=tc.bf16_grad_layers(c))
        ratios = br.check_update(net, u, f, new_w, new_b, c.lr, c.scale, c.prec)
        print("err/bound", {k: round(v, 4) for k, v in ratios.items()})
        # the check above tells the two rules apart: the `+` reference rejects the device's values
        plus = br.forward(net, S, S2, A, R, D, GAMMA, c.rule, c.prec, target=tnet)
        assert (f.live & ~f.D).sum() > c.n // 2
        with pytest.raises(AssertionError):
            br.check_q_y(plus, q_dev, y_dev, c.prec)
        assert (launches.get("gemm_qmax_screen", 0) > 0) == screened and (launches.get("qmax_refine", 0) > 0) == screened, launches
        assert (launches.get("td_target_delta", 0) == 0) == inside, launches
    finally:
        d.close()


@pytest.mark.parametrize("name", list(STEPS))
def test_zero_rewards_give_minus_the_twins_target_and_off_is_a_handle_never_asked(xq, name):
    """(b) and (c)"""
    c, huber, screened, inside = case_of(name)
    batch = batch_of(xq, c.n, c.seed)
    S, A, R, D, S2 = batch
    z, p = handle_of(xq, c, huber, True), handle_of(xq, c, huber, None)
    try:
        assert p.zero_sum() is False
        R0 = np.zeros_like(R)
        qz, yz = step(z, c, batch, R=R0, lr=0.0)
        qp, yp = step(p, c, batch, R=R0, lr=0.0)
        live, done = A >= 0, D != 0
        boot = live & ~done
        assert boot.sum() > c.n // 2 and (live & done).any()
        assert np.array_equal(bits(qz), bits(qp))
        assert (yp[boot] != 0).all() and np.array_equal(bits(yz[boot]), bits(-yp[boot]))
        assert np.array_equal(bits(yz[live & done]), bits(yp[live & done])) and (yz[live & done] == 0).all()
        assert (yz[~live] == 0).all() and (yp[~live] == 0).all()
        for x, y in zip(z.get_params(), p.get_params()):
            assert np.array_equal(x, y)
        # (c) off again: parameters, Q(s,a), y and the launches of a handle that was never asked
        z.set_zero_sum(False)
        assert z.zero_sum() is False
        z.kernel_stats(2); p.kernel_stats(2)
        qz, yz = step(z, c, batch)
        qp, yp = step(p, c, batch)
        sz, sp = z.kernel_stats(0), p.kernel_stats(0)
        assert [(s["name"], s["launches"]) for s in sz] == [(s["name"], s["launches"]) for s in sp]
        assert np.array_equal(bits(qz), bits(qp)) and np.array_equal(bits(yz), bits(yp))
        for x, y in zip(z.get_params() + z.get_params(1), p.get_params() + p.get_params(1)):
            assert np.array_equal(x, y)
        # ... and on again it is live: the next step's targets differ
        z.set_zero_sum(True)
        _, yz2 = step(z, c, batch, lr=0.0)
        _, yp2 = step(p, c, batch, lr=0.0)
        assert (yz2[boot] != yp2[boot]).all() and np.array_equal(bits(yz2[live & done]), bits(yp2[live & done]))
    finally:
        z.close(); p.close()


# ---- 2. prioritized ----------------------------------------------------------------------------------------------------------------------
def test_prioritized_priorities_follow_the_zero_sum_target(xq):
    c = tc._case("z", F64, 300, 2, 0)
    batch, lrate = 160, 0.05
    scale = 16.0 / batch
    S, A, R, D, S2 = batch_of(xq, c.n, c.seed)
    d = handle_of(xq, c, False, True)
    rp = xq.ReplayBuffer(c.n, seed=RING_SEED)
    try:
        rp.enable_per(*PER)
        rp.push(S, A, R, D, S2)
        w0, b0 = d.get_params()
        wt0, bt0 = d.get_params(1)
        prio = np.random.default_rng(5).uniform(1.0, 2.0, size=c.n).astype(np.float32)
        rp.set_priorities(prio)
        rp.per_rebuild()
        slots, weights = rp.sample_prioritized(batch)
        d.td_grads_replay(rp, batch, td_net=2, mode=c.mode)
        d.apply_grads(lrate, scale)
        q_dev, y_dev = d.last_td_values(batch)
        new_w, new_b = d.get_params()
        net, tnet = br.Net(c.sizes, w0, b0), br.Net(c.sizes, wt0, bt0)
        f = zr.forward(net, S[slots], S2[slots], A[slots], R[slots], D[slots], GAMMA, 2, target_net=tnet)
        _, y_use = br.check_q_y(f, q_dev, y_dev, br.PRECISION_F32)
        u = br.accumulate(net, f, br.backward(net, f, c.mode, br.PRECISION_F32, weights, y=y_use))
        br.check_update(net, u, f, new_w, new_b, lrate, scale, br.PRECISION_F32)
        p2 = rp.get_priorities(0, c.n)
        live = f.live
        p_dev = (np.abs(q_dev.astype(np.float64) - y_dev) + PER[2]) ** PER[0]
        assert np.allclose(p2[slots[live]], p_dev[live], rtol=2e-5, atol=0)
        e_ref = br.priorities(f, PER[2], PER[0], y=y_use) ** (1 / PER[0])
        assert np.abs(e_ref[live] - p_dev[live] ** (1 / PER[0])).max() < 2 * br.QTOL
        # the `+` rule's priorities are others
        plus = br.forward(net, S[slots], S2[slots], A[slots], R[slots], D[slots], GAMMA, 2, target=tnet)
        e_plus = br.priorities(plus, PER[2], PER[0]) ** (1 / PER[0])
        boot = live & ~f.D                       # (|q - y| of the two rules can agree where q is close to r: most rows, not all)
        assert boot.sum() > batch // 2 and (np.abs(e_plus[boot] - p_dev[boot] ** (1 / PER[0])) >= 2 * br.QTOL).mean() > 0.5
        untouched = np.setdiff1d(np.arange(c.n), slots[live])
        assert np.array_equal(bits(p2[untouched]), bits(prio[untouched]))
    finally:
        d.close(); rp.close()


# ---- 3. the legal-move bootstrap ---------------------------------------------------------------------------------------------------------
def legal_rows(golden_dir, n):
    from test_legal_gpu import pool, rows_of
    p = pool(golden_dir)
    return rows_of(p, np.arange(200, 200 + n) % p["n"])


def legal_handle(xq, zero_sum):
    from test_legal_gpu import legal_net
    d = legal_net(xq, CFG2_NET)                  # gamma 0.97
    d.set_zero_sum(zero_sum)
    return d


@pytest.mark.parametrize("n,rule", [(300, 0), (300, 2), (2048, 0), (2048, 2)])
def test_a_side_without_a_move_has_lost(xq, golden_dir, n, rule):
    """one slab (n = 300) and k-slabs (n = 2048), online and Double: zmax / a_star / n_moves on no-move, done and dead rows, y there bit
    for bit, the selection on every other row bit for bit legal_ref on the device's own z96, the fp64 rule at n = 300, and zero-sum
    off on the same batch"""
    b = legal_rows(golden_dir, n)
    g = 0.97
    skipped = (b["D"] != 0) | (b["A"] < 0)
    lens = np.array([len(x) for x in b["lists"]])
    stuck = ~skipped & (lens == 0)
    assert stuck.sum() >= 10 and (b["D"] != 0).any() and (b["A"] < 0).any() and (lens[~skipped] > 64).any()
    d, off = legal_handle(xq, True), legal_handle(xq, False)
    mode = 0 if tc.reference_mode_defined(CFG2_NET) else 1
    lrate, scale = 1.0, 16.0 / n
    try:
        w0, b0 = d.get_params()
        wt0, bt0 = d.get_params(1)
        d.kernel_stats(2)
        q, y = d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], td_net=rule, mode=mode, learning_rate=lrate, grad_scale=scale,
                           next_player=b["side"])
        launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
        assert launches.get("legal_qmax") == 1 and launches.get("gemm_legal_head") == (2 if rule == 2 else 1)
        L = d.last_legal(n)
        new_w, new_b = d.get_params()
        assert np.isneginf(L["zmax"][stuck]).all() and (L["a_star"][stuck] == -1).all() and (L["n_moves"][stuck] == 0).all()
        assert np.array_equal(L["n_moves"] == 0, stuck)
        assert (L["zmax"][skipped] == 0).all() and (L["a_star"][skipped] == -1).all() and (L["n_moves"][skipped] == -1).all()
        assert not np.isinf(L["zmax"][~stuck]).any()
        assert np.array_equal(bits(y[stuck]), bits((b["R"][stuck] + np.float32(g)).astype(np.float32)))
        done = (b["D"] != 0) & (b["A"] >= 0)
        assert np.array_equal(bits(y[done]), bits(b["R"][done])) and (y[b["A"] < 0] == 0).all()
        # the selection on the device's own values, as tests/test_legal_gpu.py holds it
        moved = ~skipped & (lens > 0)
        a, zm = lr.pick_rows(L["z96"], [x if m else x[:0] for x, m in zip(b["lists"], moved)])
        assert np.array_equal(L["n_moves"][moved], lens[moved]) and np.array_equal(L["a_star"][moved], a[moved])
        if rule == 0:                           # (Double: zmax is the target net's value of the online pick, not a z96 entry)
            assert np.array_equal(bits(L["zmax"][moved]), bits(zm[moved]))
            yr = b["R"][moved] - np.float32(g) * np.tanh(L["zmax"][moved].astype(np.float64)).astype(np.float32)
            assert np.abs(y[moved] - yr).max() < 1e-6
        if n == 300:                            # the arithmetic against fp64, tolerances of batch_ref
            net, tnet = br.Net(CFG2_NET, w0, b0), br.Net(CFG2_NET, wt0, bt0)
            f = zr.legal_forward(net, b["S"], b["S2"], b["A"], b["R"], b["D"], b["side"], g, rule, target_net=tnet, lists=b["lists"])
            assert np.array_equal(f.n_moves, L["n_moves"]) and np.array_equal(f.no_move, stuck)
            _, y_use = br.check_q_y(f, q, y, br.PRECISION_F32)
            u = br.accumulate(net, f, br.backward(net, f, mode, br.PRECISION_F32, None, y=y_use))
            br.check_update(net, u, f, new_w, new_b, lrate, scale, br.PRECISION_F32)
        # zero-sum off: the same batch gives zmax = 0 and y = r there, and the same selection everywhere
        qo, yo = off.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], td_net=rule, mode=mode, learning_rate=0.0, grad_scale=scale,
                               next_player=b["side"])
        Lo = off.last_legal(n)
        assert (Lo["zmax"][stuck] == 0).all() and np.array_equal(bits(yo[stuck]), bits(b["R"][stuck]))
        assert np.array_equal(Lo["a_star"], L["a_star"]) and np.array_equal(Lo["n_moves"], L["n_moves"])
        assert np.array_equal(bits(Lo["zmax"][~stuck]), bits(L["zmax"][~stuck])) and np.array_equal(bits(qo), bits(q))
        assert (yo[moved] != y[moved]).all()
    finally:
        d.close(); off.close()


# ---- 4. n-step ---------------------------------------------------------------------------------------------------------------------------
def sided_fixture(cap, stride, pushes, seed):
    """nstep_ref.fixture with a side byte per push; every third next board holds Red pieces only and has Black to move (no move)"""
    fx = nr.fixture(cap, stride, pushes, seed)
    rng = np.random.default_rng(seed + 1)
    side = rng.integers(0, 2, size=pushes).astype(np.uint8)
    S2 = fx["push_S2"].copy()
    lone = np.arange(pushes) % 3 == 1
    S2[lone] = np.where(S2[lone] > 7, S2[lone] - 7, S2[lone])
    side[lone] = 1
    fx["push_S2"], fx["push_side"] = S2, side
    fx["side"] = np.zeros(cap, np.uint8)
    for t in range(pushes):
        fx["S2"][t % cap], fx["side"][t % cap] = S2[t], side[t]
    return fx


def fill(xq, fx, per=False, sided=False):
    rp = xq.ReplayBuffer(fx["cap"], seed=RING_SEED)
    if sided:
        rp.track_next_player()
    if per:
        rp.enable_per(*PER)
    for t in range(0, fx["pushes"], fx["cap"]):
        e = min(t + fx["cap"], fx["pushes"])
        kw = dict(next_player=fx["push_side"][t:e]) if sided else {}
        rp.push(fx["push_S"][t:e], fx["push_A"][t:e], fx["push_R"][t:e], fx["push_D"][t:e], fx["push_S2"][t:e], **kw)
    return rp


@pytest.mark.parametrize("variant", ["alone", "mirror", "colour_swap", "legal", "prioritized"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_n_step_returns_alternate_and_the_step_is_the_one_step_step_on_the_assembled_batch(xq, n, variant):
    cap, stride, batch, lrate = 64, 4, 65, 0.05
    legal, per = variant == "legal", variant == "prioritized"
    fx = sided_fixture(cap, stride, 150, seed=13)
    rp = fill(xq, fx, per=per, sided=legal)
    disc = zr.discounts(NGAMMA, n)
    assert (float(disc[n]) < 0) == (n % 2 == 1) and abs(float(disc[n])) == float(nr.discounts(NGAMMA, n)[n])
    a, w, _ = make_net(xq, SMALL_NET, seed=8, gamma=NGAMMA)
    # the host step's discount: disc_n as the device forms it — a handle with gamma = |disc_n|, zero-sum iff disc_n < 0
    bq, _, _ = make_net(xq, SMALL_NET, seed=8, gamma=abs(float(disc[n])))
    try:
        a.set_zero_sum(True)
        bq.set_zero_sum(n % 2 == 1)
        if legal:
            a.set_td_bootstrap("legal"); bq.set_td_bootstrap("legal")
        if variant == "mirror":
            rp.set_mirror(0.5)
        if variant == "colour_swap":
            rp.set_colour_swap(0.5)
        if per:
            prio = np.random.default_rng(5).uniform(1.0, 2.0, size=cap).astype(np.float32)
            rp.set_priorities(prio)
            rp.per_rebuild()
        rp.set_n_step(n, stride)
        if legal:                                # the identity batch over the filled ring: every chain of the fixture, in slot order
            batch, slots = fx["size"], nr.filled_slots(fx)
        else:
            slots = rp.sample_prioritized(batch)[0] if per else rp.sample(batch)
        exact = not (legal or per)              # the host step has no importance weights; legal compares targets (see below)
        lr_a = lrate if exact else 0.0
        a.td_grads_replay(rp, 0 if legal else batch)
        a.apply_grads(lr_a, 1.0 / batch)
        qa, ya = a.last_td_values(batch)
        got = a.last_n_step(batch)
        first, count = nr.readable(cap, fx["size"], fx["write_pos"])
        ref = zr.assemble(fx["A"], fx["R"], fx["D"], cap, slots, n, stride, NGAMMA, first, count)
        same = nr.assemble(fx["A"], fx["R"], fx["D"], cap, slots, n, stride, NGAMMA, first, count)
        assert np.array_equal(bits(got["reward"]), bits(ref["reward"]))
        for k in ("done", "steps", "first_slot", "last_slot"):
            assert np.array_equal(got[k], ref[k]), k
        longer = got["steps"] >= 2
        assert longer.sum() > batch // 3 and (got["reward"][longer] != same["reward"][longer]).mean() > 0.9
        assert ref["dead"].any() and (ref["steps"] == n).any() and (ref["done"][~ref["dead"]] != 0).any()
        S, A, R, D, S2 = nr.staged(fx, ref)
        if variant == "mirror":
            m = a.last_mirror(batch)
            assert 0 < m["flags"].sum() < batch
            S, S2, A = m["boards"], m["next_boards"], m["action"]
        elif variant == "colour_swap":
            m = a.last_colour_swap(batch)
            assert 0 < m["flags"].sum() < batch
            S, S2, A = m["boards"], m["next_boards"], m["action"]
        else:
            assert np.array_equal(got["action"], ref["action"])
        kw = {}
        if legal:
            last = np.where(ref["dead"], ref["first_slot"], ref["last_slot"])
            kw = dict(next_player=fx["side"][last])
        qb, yb = bq.td_update(S, S2, A, R, D, learning_rate=lr_a, grad_scale=1.0 / batch, **kw)
        assert np.array_equal(bits(qa), bits(qb))
        live = A >= 0
        boot = live & (D == 0)
        if legal:
            La, Lb = a.last_legal(batch, z96=False), bq.last_legal(batch, z96=False)
            assert np.array_equal(La["n_moves"], Lb["n_moves"]) and np.array_equal(La["a_star"], Lb["a_star"])
            stuck = La["n_moves"] == 0
            assert stuck.sum() >= 3 and (La["n_moves"] > 0).sum() >= 5 and np.isneginf(La["zmax"][stuck]).all()
            # a side without a move is worth -1 whichever side it is: y = R + disc_n (-1); the twin of an even n runs without zero-sum
            # and keeps y = R there, so those rows are compared with the rule itself
            assert np.array_equal(bits(ya[stuck]), bits((R[stuck] - disc[n]).astype(np.float32)))
            assert np.array_equal(bits(ya[~stuck]), bits(yb[~stuck]))
            if n % 2 == 1:
                assert np.array_equal(bits(ya), bits(yb))
        else:
            assert np.array_equal(bits(ya), bits(yb))
        assert boot.any() and (np.abs(ya[boot].astype(np.float64) - R[boot]) <= abs(float(disc[n])) * (1 + 1e-6)).all()
        if exact:
            (wa, ba), (wb, bb) = a.get_params(), bq.get_params()
            assert np.array_equal(wa, wb) and np.array_equal(ba, bb) and np.abs(wa - w).max() > 0
        if per:
            p2 = rp.get_priorities(0, cap)
            want = (np.abs(qa.astype(np.float64) - ya) + PER[2]) ** PER[0]
            assert np.allclose(p2[slots[live]], want[live], rtol=2e-5, atol=0)
            rest = np.setdiff1d(np.arange(cap), slots[live])
            assert np.array_equal(bits(p2[rest]), bits(prio[rest]))
    finally:
        a.close(); bq.close(); rp.close()


# ---- 5. the setters ----------------------------------------------------------------------------------------------------------------------
def test_setter_errors_and_what_the_setting_survives(xq, tmp_path):
    from cn_chess_ai_amd import _capi
    from test_adam_gpu import ring
    from test_dqn_gpu import REF_NET
    d, w, b = make_net(xq, REF_NET, seed=2)
    try:
        assert d.zero_sum() is False
        for bad in (2, -1, 7):
            with pytest.raises(xq.XqError) as e:
                _capi.call("xq_dqn_set_zero_sum", d.handle, bad)
            assert e.value.code == 1
        for bad in (1, 0, "on", None, 1.0):
            with pytest.raises(ValueError):
                d.set_zero_sum(bad)
        with pytest.raises(xq.XqError) as e:
            _capi.call("xq_dqn_get_zero_sum", d.handle, None)
        assert e.value.code == 1
        assert d.zero_sum() is False
        d.set_zero_sum(True)
        path = str(tmp_path / "m.bin")
        d.saveModel(path)
        for change in (lambda: d.set_optimizer("adam"), lambda: d.set_optimizer("sgd"), lambda: d.set_params(w, b), lambda: d.loadModel(path),
                       lambda: d.updateTargetNetwork(), lambda: d.set_precision(_capi.PRECISION_BF16),
                       lambda: d.set_precision(_capi.PRECISION_F32), lambda: d.set_td_bootstrap("legal"), lambda: d.set_td_bootstrap("all"),
                       lambda: d.set_td_loss("huber", 0.5), lambda: d.set_td_loss("squared"), lambda: d.set_grad_clip(1.0),
                       lambda: d.set_grad_clip(0.0), lambda: d.set_target_tau(0.5), lambda: d.set_target_tau(0.0)):
            change()
            assert d.zero_sum() is True
        # the single-sample host loop forms the reference's target: it refuses
        x = np.zeros(1260)
        with pytest.raises(ValueError):
            d.train(x, 3, 0.5, x, False)
        # refused while a TD step waits for its apply, like its siblings
        d.set_fused_apply(True)
        n = 1024
        S, A, R, D, S2 = batch_of(xq, n, 0)
        rp = ring(xq, (S, A, R, D, S2))
        try:
            slots = rp.sample(n)
            d.td_grads_replay(rp, n, td_net=0, mode=0)
            with pytest.raises(xq.XqError) as e:
                d.set_zero_sum(False)
            assert e.value.code == 2 and "waiting" in str(e.value)
            assert d.zero_sum() is True
            d.apply_grads(1e-3, 1.0 / n)
            q, y = d.last_td_values(n)
            Rs = R[slots]
            boot = (A[slots] >= 0) & (D[slots] == 0)
            assert (np.abs(y[boot] - Rs[boot]) <= 0.99 * (1 + 1e-6)).all() and (y[boot] != Rs[boot]).all()
            d.set_zero_sum(False)
            assert d.zero_sum() is False
            d.train(x, 3, 0.5, x, False)                                            # ... and the host loop runs again
        finally:
            rp.close()
    finally:
        d.close()
