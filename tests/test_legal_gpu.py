"""The legal-move TD bootstrap (xq_dqn_set_td_bootstrap, DESIGN.md §4 "Legal-move bootstrap") on the device — `pytest -m gpu`.

1. Selection, exact: on the device's own z96 (xq_dqn_last_legal) zmax and a_star are numpy's fp32 evaluation of the rule bit for bit,
   n_moves is the reference engine's list length, and a_star is the move xq_env_selfplay_step plays on the same values at epsilon 0.
2. Arithmetic against fp64 (tests/legal_ref.py on tests/batch_ref.py, the project's tolerances): z96, Q(s,a), y, every parameter, a_star
   in the fp64 candidate set; online, target and Double rule, squared and Huber loss.
3. Step paths: the fused tail's shapes, chunk edges, no screening under `legal`, `all` again is the untouched handle's bits, refusals.
"""
import numpy as np
import pytest

import batch_ref as br
import huber_ref as hr
import legal_ref as lr
import td_edge_cases as tc
import xqoracle as xo
from test_dqn_gpu import CFG2_NET

pytestmark = pytest.mark.gpu

SMALL_NET = [1260, 64, 64, 8100]
NET_SEED = 7                                    # tests/test_legal_ref_cpu.py checks the near-tie condition for this seed
GAMMA = 0.97
KAPPA = 0.05


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def legal_net(xq, sizes, seed=NET_SEED):
    """a handle under the legal bootstrap: online net init_weights(seed), a target net that differs from it"""
    w, b = xo.init_weights(sizes, seed)
    wt, bt = xo.init_weights(sizes, seed + 92)
    bt = np.random.default_rng(seed + 91).uniform(-0.05, 0.05, size=len(bt))
    d = xq.DQN(sizes, 0.001, GAMMA, seed=seed)
    d.set_params(w, b)
    d.set_params(wt, bt, net=1)
    d.set_td_bootstrap("legal")
    return d


_pool = {}


def pool(golden_dir):
    """every row the tests draw from, built once and never written: all 320 ref_bigmoves rows (both colours of 160 boards), then 256
    ref_sparse rows that include every side without a move, then the rest of ref_sparse.  Per row: s' and its side, the reference
    engine's list, s (another board of the pool), an action, a reward, done — with done rows and dead rows (action -1) scattered."""
    if not _pool:
        bb, bs, bl = lr.fixture_rows(golden_dir, "ref_bigmoves.npz")
        sb, ss, sl = lr.fixture_rows(golden_dir, "ref_sparse.npz")
        empty = [i for i, x in enumerate(sl) if len(x) == 0]
        assert len(empty) == 40
        rest = [i for i in range(len(sl)) if len(sl[i]) > 0]
        order = empty + rest[:256 - len(empty)]
        order = list(np.random.default_rng(1).permutation(order)) + rest[256 - len(empty):]
        S2 = np.concatenate([bb, sb[order]])
        side = np.concatenate([bs, ss[order]])
        lists = bl + [sl[i] for i in order]
        n = len(S2)
        rng = np.random.default_rng(2)
        A = rng.integers(0, 90, n).astype(np.int32)
        D = (rng.random(n) < 0.1).astype(np.uint8)
        A[rng.random(n) < 0.05] = -1
        A[:6], D[:6] = [3, -1, 7, 9, 11, 13], [0, 0, 1, 0, 0, 0]              # the smallest batches see a dead and a done row too
        R = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        _pool.update(S=np.roll(S2, 5, axis=0), S2=S2, side=side, lists=lists, A=A, R=R, D=D, n=n)
    return _pool


def rows_of(p, idx):
    return dict(S=p["S"][idx], S2=p["S2"][idx], side=p["side"][idx], lists=[p["lists"][i] for i in idx], A=p["A"][idx], R=p["R"][idx],
                D=p["D"][idx], n=len(idx))


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- 1. selection, exact -----------------------------------------------------------------------------------------------------------------
def assert_selection(xq, d, b, L):
    n = b["n"]
    z = L["z96"]
    skipped = (b["D"] != 0) | (b["A"] < 0)
    want_n = np.where(skipped, -1, [len(x) for x in b["lists"]])
    assert np.array_equal(L["n_moves"], want_n)
    a, zm = lr.pick_rows(z, [x if not s else x[:0] for x, s in zip(b["lists"], skipped)])
    assert np.array_equal(L["a_star"], a)
    assert np.array_equal(bits(L["zmax"]), bits(zm))
    # the epsilon = 0 policy on the same values, boards and sides
    env = xq.VecEnv(n, seed=3)
    try:
        meta = np.zeros((n, 4), np.int32)
        meta[:, 1] = b["side"]
        env.set_state(b["S2"], meta)
        res = env.selfplay_step(np.ascontiguousarray(z[:, :90]), eps=0.0)
    finally:
        env.close()
    played = np.where(res["action"] >= 0, res["action"] % 90, -1)
    assert np.array_equal(played[~skipped], L["a_star"][~skipped])
    assert np.array_equal(res["n_moves"][~skipped], L["n_moves"][~skipped])


@pytest.mark.parametrize("first,n", [(0, 576), (0, 1), (1, 1), (0, 3), (2, 4), (0, 5), (320, 64), (300, 65)])
def test_selection_is_the_rule_on_the_devices_own_values(xq, golden_dir, first, n):
    p = pool(golden_dir)
    b = rows_of(p, np.arange(first, first + n))
    d = legal_net(xq, SMALL_NET)
    try:
        assert d.td_bootstrap() == "legal"
        q, y = d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=0.0, grad_scale=1.0, next_player=b["side"])
        L = d.last_legal(n)
        assert_selection(xq, d, b, L)
        if n == 576:
            live = L["n_moves"] > 0
            assert (L["n_moves"] > 64).sum() > 100 and (L["n_moves"] == 0).sum() >= 30 and (L["n_moves"] == -1).sum() > 40
            assert set(b["side"][live]) == {0, 1}
        # y is the rule on zmax in fp32: r on done rows and rows without a move, 0 on dead rows
        yr = np.where(b["D"] != 0, b["R"], b["R"] + np.float32(GAMMA) * np.tanh(L["zmax"].astype(np.float64)).astype(np.float32))
        yr = np.where(b["A"] < 0, 0.0, yr)
        assert np.abs(y - yr).max() < 1e-6
        stay = (L["n_moves"] <= 0) & (b["A"] >= 0)
        assert np.array_equal(bits(y[stay]), bits(b["R"][stay]))
    finally:
        d.close()


def test_ties_nonfinite_values_and_long_lists_on_a_crafted_head(xq, golden_dir):
    """output rows 0..89 all equal (every z[to] ties: entry 0 of the list wins, whichever register it sits in), then a NaN weight in one
    row (it never wins)"""
    import argmax_edge_cases as ac
    p = pool(golden_dir)
    b = rows_of(p, np.arange(0, 320))
    b["A"], b["D"] = np.abs(b["A"]), np.zeros_like(b["D"])
    for pattern in ("all_equal", "dup_sets", "nan_weight", "inf_weight", "zero_signed"):
        d = legal_net(xq, SMALL_NET)
        try:
            w, bb = xo.init_weights(SMALL_NET, NET_SEED)
            w, bb = ac.edit_head(pattern, SMALL_NET, w, bb, seed=4)
            d.set_params(w, bb)
            d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=0.0, grad_scale=1.0, next_player=b["side"])
            L = d.last_legal(320)
            assert_selection(xq, d, b, L)
            if pattern == "all_equal":
                assert np.array_equal(L["a_star"], [int(x[0]) % 90 for x in b["lists"]])
        finally:
            d.close()


# ---- 2. / 3. arithmetic against fp64 -----------------------------------------------------------------------------------------------------
def step_against_reference(xq, d, sizes, b, rule, huber=False):
    n = b["n"]
    mode = 0 if tc.reference_mode_defined(sizes) else 1
    lrate, scale = 1.0, 16.0 / n
    w0, b0 = d.get_params()
    wt0, bt0 = d.get_params(1)
    if huber:
        d.set_td_loss("huber", KAPPA)
    q_dev, y_dev = d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], td_net=rule, mode=mode, learning_rate=lrate, grad_scale=scale,
                               next_player=b["side"])
    L = d.last_legal(n)
    new_w, new_b = d.get_params()
    net, tnet = br.Net(sizes, w0, b0), br.Net(sizes, wt0, bt0)
    f = lr.forward(net, b["S"], b["S2"], b["A"], b["R"], b["D"], b["side"], GAMMA, rule, target=tnet, lists=b["lists"])
    zerr = float(np.abs(L["z96"] - f.z96).max())
    print("z96 err", zerr)
    assert zerr < br.QTOL
    assert np.array_equal(L["n_moves"], f.n_moves)
    picked = np.flatnonzero(f.n_moves > 0)
    for i in picked:
        assert L["a_star"][i] in f.cands[i], (i, L["a_star"][i], f.cands[i])
    flips = int((L["a_star"][picked] != f.astar[picked]).sum())
    print("a* flips", flips, "of", len(picked))
    assert flips <= br.MAX_FLIP_FRACTION[br.PRECISION_F32] * n
    assert (L["a_star"][f.n_moves <= 0] == -1).all()
    flipped, y_use = br.check_q_y(f, q_dev, y_dev, br.PRECISION_F32)
    weights = hr.weights(f, KAPPA, None, y=y_use) if huber else None
    bk = br.backward(net, f, mode, br.PRECISION_F32, weights, y=y_use)
    u = br.accumulate(net, f, bk)
    ratios = br.check_update(net, u, f, new_w, new_b, lrate, scale, br.PRECISION_F32)
    print("err/bound", {k: round(v, 4) for k, v in ratios.items()}, "y flips", len(flipped))
    assert np.array_equal(np.concatenate(d.get_params(1)), np.concatenate([wt0, bt0]))
    return f


@pytest.mark.parametrize("rule,huber", [(0, False), (1, False), (2, False), (0, True), (2, True)])
def test_step_matches_the_fp64_rule(xq, golden_dir, rule, huber):
    p = pool(golden_dir)
    b = rows_of(p, np.arange(200, 500))          # 120 ref_bigmoves rows, 180 ref_sparse rows with sides that have no move
    d = legal_net(xq, SMALL_NET)
    try:
        f = step_against_reference(xq, d, SMALL_NET, b, rule, huber)
        assert (f.n_moves == 0).sum() >= 10 and (f.n_moves > 64).sum() >= 40
    finally:
        d.close()


WIDE_NET = [1260, 128, 512, 8100]


@pytest.mark.parametrize("sizes,n,rule", [(CFG2_NET, 256, 0), (CFG2_NET, 300, 0), (SMALL_NET, 1024, 0), (SMALL_NET, 1025, 0),
                                          (CFG2_NET, 2047, 0), (CFG2_NET, 2048, 2), (WIDE_NET, 2048, 0), (SMALL_NET, 2048, 0),
                                          ([1260, 128, 640, 8100], 2048, 0), ([1260, 128, 896, 8100], 2048, 2),
                                          ([1260, 128, 384, 8100], 2048, 0)])
def test_step_paths(xq, golden_dir, sizes, n, rule):
    """the fused tail with whole and partial tiles; one and two layer-0 chunks, the last block of legal_qmax_kernel one wave; the head
    product whole below 2048 rows and as 4 (256-wide) and 8 (512-wide) k-slabs from there on, one slab for a 64-wide layer, 6 for 384 and
    the counts launch_gemm's rounding of the k-chunk leaves odd: 7 slabs for 640 (chunks of 96) and for 896 (chunks of 128)"""
    p = pool(golden_dir)
    b = rows_of(p, np.arange(100, 100 + n) % p["n"])
    d = legal_net(xq, sizes)
    try:
        d.kernel_stats(2)
        step_against_reference(xq, d, sizes, b, rule)
        launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
        assert launches.get("legal_qmax") == 1 and launches.get("gemm_legal_head") == (2 if rule == 2 else 1) and launches.get("td_target_delta") == 1
        assert not any(k in launches for k in ("gemm_qmax_rowmax", "gemm_qmax_screen", "qmax_refine", "colmax_reduce")), launches
    finally:
        d.close()


def test_double_rule_runs_the_head_on_both_nets(xq, golden_dir):
    p = pool(golden_dir)
    d = legal_net(xq, CFG2_NET)
    try:
        d.kernel_stats(2)
        step_against_reference(xq, d, CFG2_NET, rows_of(p, np.arange(0, 300)), 2)
        launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
        assert launches.get("legal_qmax") == 1 and launches.get("gemm_legal_head") == 2 and "gemm_qmax_rowmax" not in launches
    finally:
        d.close()


def test_a_legal_step_is_never_screened(xq, golden_dir):
    from cn_chess_ai_amd import _capi
    p = pool(golden_dir)
    b = rows_of(p, np.arange(0, 1024))
    d = legal_net(xq, SMALL_NET)
    step = lambda **kw: d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=0.0, grad_scale=1.0, **kw)
    try:
        d.set_qmax_mode(_capi.QMAX_SCREENED)
        d.set_td_bootstrap("all")
        step()                                   # this shape screens under `all`: the counters move
        s0, g0 = d.qmax_stats(), d.qmax_guard()
        assert s0[0] == 1 and s0[1] == 1024
        d.set_td_bootstrap("legal")
        d.kernel_stats(2)
        for _ in range(3):
            step(next_player=b["side"])
        launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
        assert d.qmax_stats() == s0 and d.qmax_guard() == g0
        assert launches.get("legal_qmax") == 3 and "gemm_qmax_screen" not in launches and "qmax_refine" not in launches
        d.set_td_bootstrap("all")
        step()
        assert d.qmax_stats()[0] == 2
    finally:
        d.close()


def test_all_again_has_the_bits_of_a_handle_that_was_never_switched(xq, golden_dir):
    p = pool(golden_dir)
    b = rows_of(p, np.arange(0, 300))
    a, c = legal_net(xq, CFG2_NET), legal_net(xq, CFG2_NET)
    try:
        c.set_td_bootstrap("all")
        a.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=0.0, grad_scale=1.0, next_player=b["side"])
        a.set_td_bootstrap("all")
        assert a.td_bootstrap() == "all"
        for rule in (0, 2):
            # a sided call under `all` is the unsided call
            qa, ya = a.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], td_net=rule, learning_rate=0.5, grad_scale=1.0 / 300,
                                 next_player=b["side"] if rule == 0 else None)
            qc, yc = c.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], td_net=rule, learning_rate=0.5, grad_scale=1.0 / 300)
            assert np.array_equal(bits(qa), bits(qc)) and np.array_equal(bits(ya), bits(yc))
            for x, y in zip(a.get_params(), c.get_params()):
                assert np.array_equal(x, y)
        with pytest.raises(xq._capi.XqError) as e:       # the last step was not a legal one
            a.last_legal(1)
        assert e.value.code == 2
    finally:
        a.close(); c.close()


def test_facade_setter_round_trips_and_a_sided_step_runs(xq):
    import json
    import subprocess
    from test_legal_ref_cpu import build_legal_facade_probe
    exe = build_legal_facade_probe()
    out = subprocess.run([exe, "7"], check=True, capture_output=True, text=True, timeout=120).stdout
    lines = out.strip().splitlines()
    tr, r = json.loads(lines[-2]), json.loads(lines[-1])
    assert tr["train_ring_finite"] == 1 and tr["train_ring_updates"] > 0            # a short batched train() under legal()
    assert tr["train_onpolicy_finite"] == 1 and tr["train_onpolicy_updates"] > 0
    assert (r["before"], r["after"], r["back"]) == (0, 1, 0)
    assert r["unknown_refused"] == 1 and r["unsided_refused"] == 1 and r["finite"] == 1
    assert (r["moves_red"], r["moves_black"]) == (44, 44)                     # the start position
    assert 0 <= r["astar_red"] < 90 and 0 <= r["astar_black"] < 90 and r["astar_red"] != r["astar_black"]
    assert abs(r["y_red"] - (0.5 + 0.99 * np.tanh(r["zmax_red"]))) < 1e-6


def test_refusals(xq, golden_dir):
    from cn_chess_ai_amd import _capi
    p = pool(golden_dir)
    b = rows_of(p, np.arange(0, 64))
    d = legal_net(xq, CFG2_NET)
    rp = xq.ReplayBuffer(64, seed=1)
    try:
        before = d.get_params()
        with pytest.raises(ValueError):
            d.set_td_bootstrap("some")
        with pytest.raises(_capi.XqError) as e:          # unsided calls under `legal`
            d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=1.0)
        assert e.value.code == 1 and "side to move" in str(e.value)
        rp.push(b["S"], np.abs(b["A"]), b["R"], b["D"], b["S2"])
        with pytest.raises(_capi.XqError) as e:
            d.td_grads_replay(rp, 0)
        assert e.value.code == 1 and "side to move" in str(e.value)
        side = b["side"].copy(); side[5] = 2
        with pytest.raises(_capi.XqError) as e:
            d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=1.0, next_player=side)
        assert e.value.code == 1 and "next_player[5]" in str(e.value)
        for prec in (_capi.PRECISION_BF16, _capi.PRECISION_BF16_FULL):
            d.set_precision(prec)
            with pytest.raises(_capi.XqError) as e:
                d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=1.0, next_player=b["side"])
            assert e.value.code == 1 and "fp32" in str(e.value)
        d.set_precision(_capi.PRECISION_F32)
        for got, want in zip(d.get_params(), before):
            assert np.array_equal(got, want)
        with pytest.raises(_capi.XqError) as e:          # no legal step has run yet
            d.last_legal(1)
        assert e.value.code == 2
        d.td_update(b["S"], b["S2"], b["A"], b["R"], b["D"], learning_rate=0.0, next_player=b["side"])
        assert len(d.last_legal(64, z96=False)) == 3
        with pytest.raises(_capi.XqError) as e:
            d.last_legal(65)
        assert e.value.code == 1
    finally:
        rp.close(); d.close()
