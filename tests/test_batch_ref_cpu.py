"""tests/batch_ref.py, the batched fp64 TD-step reference of the full-size GPU checks: equal to the scalar oracle on every combination
it defines, and its comparator tight enough to reject the bugs full-size batches can hide (a dropped chunk or sample, a ragged tail,
the other backprop mode)."""
import os

import numpy as np
import pytest

import batch_ref as br
import infer_edge_cases as ic
import td_edge_cases as tc
import xqoracle as xo
from test_dqn_gpu import transitions, valid_indices

REF_NET = [1260, 128, 8100]
CFG2_NET = [1260, 256, 256, 8100]
CFG4_NET = [1260, 512, 512, 512, 8100]
SMALL_NET = [40, 24, 24, 56]


@pytest.fixture(scope="module")
def trace(golden_dir):
    return np.load(os.path.join(golden_dir, "ref_trace.npz"))


def _params(sizes, seed):
    w, _ = xo.init_weights(sizes, seed)
    b = np.random.default_rng(seed + 100).uniform(-0.05, 0.05, size=xo.nn_counts(sizes)[1])
    return w * 4.0, b                     # wider pre-activations: hidden deltas well away from zero


def _batch(trace, sizes, n, seed):
    S, A, R, D, S2 = transitions(trace, valid_indices(trace, n, seed=seed))
    R = (R / 1000.0).astype(np.float32)
    if sizes[0] != 1260:                  # dense inputs for the small net; actions below its width
        rng = np.random.default_rng(seed)
        S, S2 = rng.uniform(-1, 1, (n, sizes[0])), rng.uniform(-1, 1, (n, sizes[0]))
        A = (A % sizes[-1]).astype(np.int32)
    return S, A, R, D, S2


def _x(s):
    return xo.state_repr(xo.board_from(s)) if s.dtype == np.uint8 else np.asarray(s, np.float64)


def _close(got, want, what):
    scale = max(np.abs(want).max(), 1e-300)
    assert np.abs(got - want).max() <= 1e-12 * scale, (what, float(np.abs(got - want).max() / scale))


@pytest.mark.parametrize("sizes", [REF_NET, CFG2_NET, CFG4_NET, SMALL_NET], ids=["ref", "cfg2", "cfg4", "small"])
@pytest.mark.parametrize("mode", [0, 1])
def test_batched_reference_equals_the_oracle(trace, sizes, mode):
    """Q, y, a*, the activations and every gradient element against xo.ext_td_accum for TD rules 0 / 1 / 2, precisions 0 / 1 / 2,
    with and without importance weights; and against xo.td_target + xo.nn_accum_grad where that is defined (rule 0, fp32, no weights)."""
    n = 32 if sizes != CFG4_NET else 12
    S, A, R, D, S2 = _batch(trace, sizes, n, seed=3)
    assert D.any() and not D.all()
    w, b = _params(sizes, 5)
    wt, bt = _params(sizes, 6)
    wts = np.random.default_rng(1).uniform(0.1, 1.0, n)
    xs, x2s = [_x(s) for s in S], [_x(s) for s in S2]
    for prec in (0, 1, 2):
        for rule in (0, 1, 2):
            weighted = [False, True] if sizes != CFG4_NET else [(rule + prec) % 2 == 1]
            for use_w in weighted:
                net, f, bk, u = br.td_step(sizes, w, b, S, S2, A, R, D, 0.99, rule, mode, prec, wts if use_w else None, wt, bt)
                gw, gb = br.flat_grads(net, u)
                ow, ob = np.zeros_like(w), np.zeros_like(b)
                q, y, star = np.empty(n), np.empty(n), np.empty(n, np.int64)
                for i in range(n):
                    q[i], y[i], star[i] = xo.ext_td_accum(sizes, w, b, wt, bt, xs[i], x2s[i], int(A[i]), float(R[i]), int(D[i]), 0.99,
                                                          rule, mode, prec, float(wts[i]) if use_w else 1.0, ow, ob)
                key = (prec, rule, use_w)
                _close(f.q, q, ("q",) + key); _close(f.y, y, ("y",) + key)
                assert np.array_equal(f.astar, star), key
                _close(gw, ow, ("gw",) + key); _close(gb, ob, ("gb",) + key)
                for l in range(net.nl):                 # every layer's block on its own scale as well
                    blk = slice(net.wo[l], net.wo[l] + sizes[l] * sizes[l + 1])
                    _close(gw[blk], ow[blk], ("gw", l) + key)
                if rule == 2:
                    for i in np.nonzero(~f.D)[0]:
                        assert np.abs(f.cand_y[i] - y[i]).min() <= 1e-12
                if rule == 0 and not use_w:
                    acts, z = xo.ext_forward(sizes, w, b, xs[0], bf16=prec > 0)
                    _close(np.concatenate([a[0] for a in f.acts]), acts, ("acts",) + key)
                    _close(np.tanh(z[A[0]]), f.q[0], ("z",) + key)
                if rule == 0 and prec == 0 and not use_w:
                    nw, nb = np.zeros_like(w), np.zeros_like(b)
                    for i in range(n):
                        tq = xo.td_target(sizes, w, b, xs[i], x2s[i], int(A[i]), float(R[i]), int(D[i]), 0.99)
                        assert xo.nn_accum_grad(sizes, w, b, xs[i], tq, mode, nw, nb) == 0
                        assert abs(tq[A[i]] - f.y[i]) <= 1e-12 * max(1.0, abs(f.y[i]))
                    _close(gw, nw, ("nn gw", mode)); _close(gb, nb, ("nn gb", mode))
                assert abs(br.loss(f) - 0.5 * np.sum((q - y) ** 2)) <= 1e-12 * max(br.loss(f), 1e-300)


@pytest.mark.parametrize("sizes", [CFG2_NET, CFG4_NET, SMALL_NET], ids=["cfg2", "cfg4", "small"])
@pytest.mark.parametrize("mode", [0, 1])
def test_named_bf16_layers_span_bf16_full_to_bf16(trace, sizes, mode):
    """backward / accumulate with the layers of the bf16 backward products named (the device rounds by shape): every hidden
    layer named is the oracle's PRECISION_BF16_FULL, none named its PRECISION_BF16 — the two share their forward half."""
    n = 12
    S, A, R, D, S2 = _batch(trace, sizes, n, seed=4)
    w, b = _params(sizes, 5)
    wt, bt = _params(sizes, 6)
    xs, x2s = [_x(s) for s in S], [_x(s) for s in S2]
    net = br.Net(sizes, w, b, 2)
    f = br.forward(net, S, S2, A, R, D, 0.99, 2, 2, target=br.Net(sizes, wt, bt, 2))
    every = set(range(net.nl - 1))
    for layers, prec in ((every, 2), ((), 1)):
        u = br.accumulate(net, f, br.backward(net, f, mode, 2, bf16_layers=layers), 2, bf16_layers=layers)
        gw, gb = br.flat_grads(net, u)
        ow, ob = np.zeros_like(w), np.zeros_like(b)
        for i in range(n):
            xo.ext_td_accum(sizes, w, b, wt, bt, xs[i], x2s[i], int(A[i]), float(R[i]), int(D[i]), 0.99, 2, mode, prec, 1.0, ow, ob)
        _close(gw, ow, ("gw", prec)); _close(gb, ob, ("gb", prec))
    if net.nl >= 4:                                   # ... and a set in between is neither
        some = br.accumulate(net, f, br.backward(net, f, mode, 2, bf16_layers={0}), 2, bf16_layers={1})
        assert not np.array_equal(some.gW[0], u.gW[0]) and not np.array_equal(some.gW[1], u.gW[1])
    with pytest.raises(AssertionError):
        br.backward(net, f, mode, 1, bf16_layers={0})


def test_undefined_topology_is_an_error_in_both():
    sizes = [40, 16, 32, 56]                    # mode 0 reads delta_{l+1} past its end (the oracle's -1)
    w, b = _params(sizes, 2)
    x = np.random.default_rng(0).uniform(-1, 1, (3, 40))
    gw, gb = np.zeros_like(w), np.zeros_like(b)
    assert xo.nn_accum_grad(sizes, w, b, x[0], np.zeros(56), 0, gw, gb) == -1
    net = br.Net(sizes, w, b)
    f = br.forward(net, x, x, [1, 2, 3], [0.0, 0.0, 0.0], [0, 0, 1], 0.99, 0)
    with pytest.raises(br.UndefinedTopology):
        br.backward(net, f, 0)
    br.backward(net, f, 1)


def test_bf16_round_matches_the_oracle():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(3000) * 10.0 ** rng.integers(-30, 30, 3000), [0.0, -0.0, np.inf, -np.inf, np.nan, 3.3895314e38,
                        1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -9]]).astype(np.float32)
    want = np.array([xo.lib().xqo_bf16_round(float(x)) for x in v], np.float32)
    got = br.bf16_round(v).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ negative controls
def _full_batch(trace, n, seed):
    """n transitions of the reference trace drawn with replacement (rewards /100), every 9th terminal"""
    S, A, R, D, S2 = transitions(trace, valid_indices(trace, 600, seed=seed))
    pick = np.random.default_rng(seed).integers(0, len(S), n)
    D = D[pick].copy()
    D[::9] = 1
    return S[pick], A[pick], (R[pick] * 10.0 / 1000.0).astype(np.float32), D, S2[pick]


def _worst(net, u_ref, gw, gb, lr, scale, prec):
    """max err / bound when a device had computed the gradient (gw, gb) and stored the result in fp32"""
    new_w = (net.w - lr * scale * gw).astype(np.float32).astype(np.float64)
    new_b = (net.b - lr * scale * gb).astype(np.float32).astype(np.float64)
    return br.update_ratios(net, u_ref, new_w, new_b, lr, scale, prec)


def _controls(net, f, bk, prec, lr, scale, chunk, ragged, extra=()):
    n = f.n
    u = br.accumulate(net, f, bk, prec)
    gw, gb = br.flat_grads(net, u)
    ok = _worst(net, u, gw, gb, lr, scale, prec)
    assert max(ok.values()) <= 0.5, ok                                 # the reference passes its own bound: only its fp32 store rounds
    variants = {}
    m = np.ones(n, bool); m[chunk:2 * chunk] = False
    variants["one chunk missing"] = br.accumulate(net, f, bk, prec, mask=m)
    lone = int(np.nonzero(~f.D)[0][-1])
    m = np.ones(n, bool); m[lone] = False
    variants["one sample missing"] = br.accumulate(net, f, bk, prec, mask=m)
    if ragged:
        nr = n - 37                                                    # ragged n; its last n mod 64 samples dropped
        keep = np.arange(n) < nr
        u_r = br.accumulate(net, f, bk, prec, mask=keep)
        variants["ragged tail missing"] = (u_r, br.accumulate(net, f, bk, prec, mask=np.arange(n) < nr - nr % 64))
    variants["other backprop mode"] = br.accumulate(net, f, br.backward(net, f, 1 - bk.mode, prec, bk.weights), prec)
    variants.update(extra)
    seen = {}
    for name, v in variants.items():
        ref = u
        if isinstance(v, tuple):
            ref, v = v
        r = _worst(net, ref, *br.flat_grads(net, v), lr, scale, prec)
        seen[name] = max(r.values())
        if name == "one sample missing":
            # visible in the W0 columns of its board, and in fp32 in the output row of its action as well (the bf16 modes' output
            # layer carries the bf16 forward's Q error in its budget)
            assert r["w0"] >= 4.0 and (prec != 0 or r[f"w{net.nl - 1}"] >= 4.0), (name, r)
    return seen


def test_comparator_rejects_full_size_bugs_fp32(trace):
    """CFG2, n = 8192, fp32, online rule, mode 0 (the bench headline's arithmetic)."""
    sizes, n, lr, scale = CFG2_NET, 8192, 1.0, 16.0 / 8192
    S, A, R, D, S2 = _full_batch(trace, n, seed=11)
    w, b = _params(sizes, 7)
    w, b = w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    net = br.Net(sizes, w, b)
    f = br.forward(net, S, S2, A, R, D, 0.99, 0)
    bk = br.backward(net, f, 0)
    bk.mode = 0
    seen = _controls(net, f, bk, 0, lr, scale, 1024, ragged=True)
    assert min(seen.values()) >= 4.0, seen


def test_comparator_rejects_full_size_bugs_bf16_full(trace):
    """CFG4, n = 16384, bf16 everywhere (precision 2), Double DQN, importance weights (config 5's arithmetic)."""
    sizes, n, lr, scale, prec = CFG4_NET, 16384, 1.0, 16.0 / 16384, 2
    S, A, R, D, S2 = _full_batch(trace, n, seed=12)
    w, b = _params(sizes, 8)
    wt, bt = _params(sizes, 9)
    w, b = w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    wts = np.random.default_rng(2).uniform(0.2, 1.0, n)
    net = br.Net(sizes, w, b, prec)
    tnet = br.Net(sizes, wt, bt, prec)
    f = br.forward(net, S, S2, A, R, D, 0.99, 2, prec, target=tnet)
    bk = br.backward(net, f, 0, prec, wts)
    bk.mode = 0
    # the fp32 forward (no bf16 rounding) under the same backward
    net32 = br.Net(sizes, w, b, 0)
    f32 = br.forward(net32, S, S2, A, R, D, 0.99, 2, prec, target=br.Net(sizes, wt, bt, 0))
    u32 = br.accumulate(net32, f32, br.backward(net32, f32, 0, prec, wts), prec)
    seen = _controls(net, f, bk, prec, lr, scale, 2048, ragged=False, extra={"fp32 forward": u32})
    assert min(seen.values()) >= 4.0, seen


# --------------------------------------------------------------------------------- negative control of the shape-edge cases
def _ragged_layer(sizes):
    """index k >= 1 of the widest layer width that is no multiple of 128 among the hidden layers (all multiples: the widest)"""
    hidden = list(range(1, len(sizes) - 1))
    pool = [k for k in hidden if sizes[k] % 128] or hidden
    return max(pool, key=lambda k: sizes[k])


@pytest.mark.parametrize("name", [k for k, c in tc.CASES.items() if c.rule == 2])
def test_edge_case_double_dqn_near_ties_leave_room_under_the_flip_cap(trace, name):
    """A precondition of the Double DQN edge cases, weaker than the cap itself: check_q_y asserts on the device that at most
    MAX_FLIP_FRACTION of the samples take another near-maximal action's y.  Here, on the reference trace with the case's net (the device
    cases draw self-play boards of their own), the samples whose two largest online outputs lie within 5e-4 stay under that cap.  5e-4:
    the device sums the same bf16 operands in fp32 (~1e-5 off at K = 256), and a hidden sum that close to a bf16 rounding boundary moves
    its activation by one bf16 ulp, an output by up to 0.06 * 2^-8 = 2.3e-4; two of those.  Within CAND_MARGIN = 5e-3 itself, which
    is set at the full-size nets, a third of the samples of a freshly initialised 256-256 net have a second candidate (107 of 300), so
    that count cannot be kept under the cap by choosing seeds."""
    c = tc.CASES[name]
    S, A, R, D, S2 = _full_batch(trace, c.n, seed=20 + c.seed)
    w, _ = xo.init_weights(c.sizes, 21 + c.seed)
    b = np.random.default_rng(21 + c.seed + 100).uniform(-0.05, 0.05, size=xo.nn_counts(c.sizes)[1])
    net = br.Net(c.sizes, w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64), c.prec)
    zn = net.z_out(net.hidden(br.one_hot(S2))[-1])
    top2 = np.partition(zn, -2, axis=1)[:, -2:]
    ties = int(((top2[:, 1] - top2[:, 0] < 5e-4) & (D == 0)).sum())
    assert ties <= br.MAX_FLIP_FRACTION[c.prec] * c.n, (ties, c.n)


@pytest.mark.parametrize("name", tc.CONTROL)
def test_edge_case_bound_rejects_a_dropped_sample_and_a_dropped_column(trace, name):
    """One case of each family of tests/td_edge_cases.py (the table tests/test_td_shape_edges_gpu.py runs on the device), with the
    case's net seed, lr and scale: the fp64 update stored in fp32 passes check_update; the update without the batch's last sample, and
    the one whose gradient misses its last column at the widest ragged width (what a wrong mask on a last partial tile loses), do not."""
    c = tc.CASES[name]
    sizes, n, prec = c.sizes, c.n, c.prec
    S, A, R, D, S2 = _full_batch(trace, n, seed=20 + c.seed)
    D[-1] = 0
    w, _ = xo.init_weights(sizes, 21 + c.seed)                        # test_dqn_gpu.make_net's parameters, as the device stores them
    b = np.random.default_rng(21 + c.seed + 100).uniform(-0.05, 0.05, size=xo.nn_counts(sizes)[1])
    wt, _ = xo.init_weights(sizes, 99 + c.seed)
    bt = np.random.default_rng(98 + c.seed).uniform(-0.05, 0.05, size=len(b))
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    net = br.Net(sizes, f32(w), f32(b), prec)
    f = br.forward(net, S, S2, A, R, D, 0.99, c.rule, prec, target=br.Net(sizes, f32(wt), f32(bt), prec) if c.rule else None)
    dl, gl = tc.bf16_delta_layers(c), tc.bf16_grad_layers(c)
    bk = br.backward(net, f, c.mode, prec, bf16_layers=dl)
    u = br.accumulate(net, f, bk, prec, bf16_layers=gl)

    def check(gw, gb):
        ls = c.lr * c.scale
        return br.check_update(net, u, f, f32(net.w - ls * gw), f32(net.b - ls * gb), c.lr, c.scale, prec)

    gw, gb = br.flat_grads(net, u)
    ok = check(gw, gb)
    assert max(ok.values()) <= 0.5, ok                                # only the fp32 store rounds
    keep = np.ones(n, bool); keep[-1] = False
    with pytest.raises(AssertionError, match="outside the bound"):
        check(*br.flat_grads(net, br.accumulate(net, f, bk, prec, mask=keep, bf16_layers=gl)))
    k = _ragged_layer(sizes)
    gw2 = gw.copy()
    gw2[net.wo[k]:net.wo[k] + sizes[k] * min(sizes[k + 1], u.gW[k].shape[0])].reshape(-1, sizes[k])[:, -1] = 0.0
    with pytest.raises(AssertionError, match="outside the bound"):
        check(gw2, gb)


# ------------------------------------------------------------------------------------------------ the inference rows (q_rows)
@pytest.mark.parametrize("sizes", [REF_NET, [1260, 127, 129, 132, 8100], [1260, 100, 132, 8100], SMALL_NET], ids=["ref", "odd3", "even2", "small"])
def test_q_rows_equals_the_oracle(trace, sizes):
    """batch_ref.q_rows against xo.nn_forward (fp32 nets) and tanh of xo.ext_forward(..., bf16=True)'s z (the bf16 Q-net arithmetic): an
    odd-width net with three hidden layers, boards and dense inputs, all outputs and the first 90 / 96 / 1."""
    n = 9
    rng = np.random.default_rng(2)
    x = trace["board"][rng.choice(len(trace["board"]), n, replace=False)] if sizes[0] == 1260 else rng.uniform(-1, 1, (n, sizes[0]))
    w, b = _params(sizes, 11)
    for prec in (0, 1):
        net = br.Net(sizes, w, b, prec)
        if prec == 0:
            want = np.stack([xo.nn_forward(sizes, w, b, _x(s)) for s in x])
        else:
            want = np.tanh(np.stack([xo.ext_forward(sizes, w, b, _x(s), bf16=True)[1] for s in x]))
        for n_out in (sizes[-1], 1, 90 if sizes[-1] >= 96 else 7, 96 if sizes[-1] >= 96 else 56):
            got = br.q_rows(net, x, n_out, chunk=4)                   # three chunks, the last one ragged
            assert got.shape == (n, n_out)
            _close(got, want[:, :n_out], ("q_rows", prec, n_out))
        if sizes[0] == 1260:                                          # a board and its one-hot rows are the same input
            assert np.array_equal(br.q_rows(net, br.one_hot(x), 96), br.q_rows(net, x, 96))


# --------------------------------------------------------------------- negative controls of the inference cases (infer_edge_cases)
_cpu_positions = {}


def oracle_positions(n=2048, plies=25, seed=0x5EED):
    """(boards, side to move, legal destinations) of n games after `plies` uniform-random plies of the oracle's self-play loop: what
    xq_trainer_random_plies leaves on the device for the same seed (tests/test_env_gpu.py pins the two loops to each other)"""
    key = (n, plies, seed)
    if key not in _cpu_positions:
        S, P, dests = np.zeros((n, 90), np.uint8), np.zeros(n, np.int64), []
        for g in range(n):
            b, k = xo.new_board(), 0
            for _ in range(plies):
                k += int(xo.selfplay_step(b, None, seed, g, k, 0).action_code >= 0)
            S[g], P[g] = b.squares(), b.currentPlayer
            codes, cnt = xo.all_valid_actions(b, b.currentPlayer)
            dests.append(codes[:cnt].astype(np.int64) % 90)
        _cpu_positions[key] = (S, P, dests)
    return _cpu_positions[key]


def _infer_net(c):
    """test_dqn_gpu.make_net's parameters for the case with the output layer scaled, as the device stores them"""
    w, _ = xo.init_weights(c.sizes, 21 + c.seed)
    b = np.random.default_rng(21 + c.seed + 100).uniform(-0.05, 0.05, size=xo.nn_counts(c.sizes)[1])
    w[br.offsets(c.sizes)[0][-1]:] *= c.wscale
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    return br.Net(c.sizes, f32(w), f32(b), c.prec)


def _infer_boards(c):
    S = oracle_positions()[0]
    return S[np.arange(c.n) % len(S)]


def _after_layer0(net, z1):
    """the last hidden activations from the layer-0 sums z1 (bias included)"""
    rnd = br.bf16_round if net.bf else (lambda v: v)
    a = rnd(np.tanh(z1))
    for l in range(1, net.nl - 1):
        a = rnd(np.tanh(net.Bf[l] + a @ net.Wf[l].T))
    return a


def _head_damages(net, a_last, n_out, j):
    """name -> Q rows [n][n_out] the way a wrong head would leave them; "right" is q_rows"""
    W, B = net.Wf[-1][:n_out], net.Bf[-1][:n_out]
    z = B + a_last @ W.T
    two = min(128, a_last.shape[1])
    out = {"right": z, "one 64-column k-slab left out": z - a_last[:, :64] @ W[:, :64].T, "rows shifted by one sample": np.roll(z, 1, axis=0)}
    out["two slabs of one output summed twice"] = z.copy()
    out["two slabs of one output summed twice"][:, j] += a_last[:, :two] @ W[j, :two]
    out["the bias of one output dropped"] = z.copy()
    out["the bias of one output dropped"][:, j] -= B[j]
    return {k: np.tanh(v) for k, v in out.items()}


def _derived_damages(net, prev, cur):
    """name -> layer-0 sums of `cur` derived from those of `prev` the way a wrong kernel would: the take-out row of the first changed
    square that held a piece skipped (every row with such a square), and the 9th pair dropped (rows with exactly 9 differences, had the
    kernel derived them instead of summing in full)"""
    z = net.Bf[0] + br.one_hot(cur) @ net.Wf[0].T
    skip, ninth = z.copy(), z.copy()
    hit = [0, 0]
    for i in range(len(cur)):
        diff = np.nonzero(prev[i] != cur[i])[0]
        held = [s for s in diff if prev[i, s]]
        if held and len(diff) <= 8:
            skip[i] += net.Wf[0][:, held[0] * 14 + int(prev[i, held[0]]) - 1]
            hit[0] += 1
        if len(diff) == 9:
            s = diff[8]
            if prev[i, s]:
                ninth[i] += net.Wf[0][:, s * 14 + int(prev[i, s]) - 1]
            if cur[i, s]:
                ninth[i] -= net.Wf[0][:, s * 14 + int(cur[i, s]) - 1]
            hit[1] += 1
    assert min(hit) > 0
    return {"a take-out row skipped": skip, "the 9th pair dropped": ninth}


@pytest.mark.parametrize("name", [k for k in ic.CONTROL if ic.CASES[k].kind in ("boards", "select", "dense")])
def test_inference_bar_rejects_a_wrong_head_and_a_wrong_derived_sum(name):
    """One case of families A, B, D and E of tests/infer_edge_cases.py with the case's net: the fp64 rows stored in fp32 pass the case's
    bar; a head without one k-slab, with two slabs of one output summed twice, with the rows shifted by one sample or without one
    output's bias does not; for the select chain neither do rows whose derived layer-0 sum skipped a take-out row or dropped its 9th pair
    (against the wider bar of derived rows)."""
    c = ic.CASES[name]
    net = _infer_net(c)
    S = _infer_boards(c)
    x = S
    if c.kind == "dense":
        x = br.one_hot(S)
        x[-32:] = np.random.default_rng(c.seed).uniform(-1, 1, size=(32, c.sizes[0]))
    bar = br.BF16_QTOL if c.prec else ic.BAR_F32
    want = br.q_rows(net, x, c.n_out)
    a_last = net.hidden(br.one_hot(x))[-1]
    assert np.array_equal(_after_layer0(net, net.Bf[0] + br.one_hot(x) @ net.Wf[0].T), a_last)
    j = int(np.argmax(np.abs(net.Bf[-1][:c.n_out])))
    assert abs(net.Bf[-1][j]) > (1e-3 if not c.prec else 2e-2)
    for what, q in _head_damages(net, a_last, c.n_out, j).items():
        err = float(np.abs(q.astype(np.float32).astype(np.float64) - want).max())
        assert (err < 0.1 * bar) if what == "right" else (err > bar), (what, err, bar)
    if c.kind == "select":
        cur, nds = ic.edit_boards(S, 2, c.seed)
        want = br.q_rows(net, cur, c.n_out)
        for what, z1 in _derived_damages(net, S, cur).items():
            q = np.tanh(net.Bf[-1][:c.n_out] + _after_layer0(net, z1) @ net.Wf[-1][:c.n_out].T)
            err = np.abs(q - want).max(axis=1)
            assert err.max() > ic.BAR_DERIVED and (err[nds == 0] == 0).all(), (what, float(err.max()))


def test_td_bound_rejects_a_wrong_head_and_a_wrong_derived_sum():
    """Family F's control: Q(s,a) and y of the crafted (S, S2) pairs from a damaged head of s' or s, or from a damaged derived layer-0
    sum of s', leave check_q_y's bound; the undamaged ones stored in fp32 pass it."""
    c = ic.CASES[[k for k in ic.CONTROL if ic.CASES[k].kind == "td"][0]]
    net = _infer_net(c)
    S = _infer_boards(c)
    S2, nds = ic.edit_boards(S, 0, c.seed)
    rng = np.random.default_rng(c.seed + 5)
    A = rng.integers(0, 90, c.n).astype(np.int32)
    R = rng.uniform(-0.5, 0.5, c.n).astype(np.float32)
    D = np.zeros(c.n, np.uint8)
    f = br.forward(net, S, S2, A, R, D, 0.99, 0, c.prec)
    NO = c.sizes[-1]
    a_s, a_s2 = net.hidden(br.one_hot(S))[-1], net.hidden(br.one_hot(S2))[-1]
    j = int(A[np.argmax(np.abs(net.Bf[-1][A]))])
    assert abs(net.Bf[-1][j]) > 1e-3

    def q_y(qs, qs2):
        return qs[np.arange(c.n), A].astype(np.float32), (R + 0.99 * qs2.max(axis=1)).astype(np.float32)

    ds, ds2 = _head_damages(net, a_s, NO, j), _head_damages(net, a_s2, NO, j)
    br.check_q_y(f, *q_y(ds["right"], ds2["right"]), c.prec)
    for what in ds:
        if what == "right":
            continue
        for qs, qs2 in ((ds[what], ds2["right"]), (ds["right"], ds2[what])):
            if what in ("two slabs of one output summed twice", "the bias of one output dropped") and qs2 is not ds2["right"]:
                continue                                              # one output of s' shows in y only where it is the maximum
            with pytest.raises(AssertionError):
                br.check_q_y(f, *q_y(qs, qs2), c.prec)
    for what, z1 in _derived_damages(net, S, S2).items():
        qs2 = np.tanh(net.z_out(_after_layer0(net, z1)))
        with pytest.raises(AssertionError):
            br.check_q_y(f, *q_y(ds["right"], qs2), c.prec)


@pytest.mark.parametrize("name", [k for k, c in ic.CASES.items() if c.kind == "collect"])
def test_collect_cases_have_a_clear_best_move_in_the_reference_alone(name):
    """The precondition of family C's third check, without a device: on the oracle's positions after 25 random plies (the trainer's, for
    the case's seed) with the oracle's move generator and q_rows, the games whose best legal destination leads the runner-up by more than
    2 x 5e-6 are at least 95 % of the 2048; the first best move in list order passes the move checks, and the moves chosen from Q rows
    shifted by one game do not.  (The versus case plays from these positions one opponent half-ply later in the games it opens.)"""
    c = ic.CASES[name]
    S, P, dests = oracle_positions(c.n, 25, 0x5EED + c.seed)
    q = br.q_rows(_infer_net(c), S, 90)

    def greedy(rows):
        return np.array([d[np.argmax(rows[g, d])] if len(d) else -1 for g, d in enumerate(dests)], np.int64)

    clear, bad = ic.move_checks(q, greedy(q), dests, ic.BAR_F32)
    assert not bad, bad[:3]
    assert clear >= 0.95 * c.n, clear
    _, bad = ic.move_checks(q, greedy(np.roll(q, 1, axis=0)), dests, ic.BAR_F32)
    assert len(bad) > 0.5 * c.n, len(bad)
