"""Every inference path of the Q-net at its kernel-selection boundaries against the fp64 rows of tests/batch_ref.py — `pytest -m gpu`.

The Q-values everything acts on come from xq_dqn_forward_boards_dev (the arena and the versus opponent), xq_dqn_select_q_dev and
xq_trainer_collect (the self-play select chain, the env kernel finishing the head), the dense xq_dqn_forward and the derived s' chain
of a TD step; about fifteen shape predicates pick their kernels.  The table of tests/infer_edge_cases.py puts one small case on each
side of each of them.  Every element of every row is compared with batch_ref.q_rows; nothing is sampled; the bars are the project's own
(infer_edge_cases: 5e-6 / 2e-5 / BF16_QTOL / TOLERANCES).  Where the kernel_stats brackets tell two paths apart the case asserts the
one it was written for.  Largest error per case on an MI355X: profiles/NOTES.md ("Inference at the kernel-selection boundaries").
"""
import ctypes as C

import numpy as np
import pytest

import batch_ref as br
import infer_edge_cases as ic
import td_edge_cases as tc
from test_batch_ref_cpu import oracle_positions
from test_dqn_gpu import make_net
from test_td_full_size_gpu import selfplay_batch
from test_td_shape_edges_gpu import net_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


_boards = {}


def boards_of(xq, n, seed):
    """self-play positions after 20-40 random plies, as selfplay_batch draws them; shared by the cases, never written"""
    if (n, seed) not in _boards:
        _boards[(n, seed)] = selfplay_batch(xq, n, seed=3000 + n + seed, plies=20 + (n + seed) % 21, every=7)[0]
    return _boards[(n, seed)]


def handle_of(xq, c):
    """make_net's handle for the case, its output layer scaled by c.wscale; returns (handle, the reference Net of what the device holds)"""
    d, w, b = make_net(xq, c.sizes, seed=21 + c.seed)
    if c.wscale != 1.0:
        w[br.offsets(c.sizes)[0][-1]:] *= c.wscale
        d.set_params(w, b)
        d.updateTargetNetwork()
    d.set_precision(c.prec)
    d.set_l0_derive(True)
    w0, b0 = d.get_params()
    return d, br.Net(c.sizes, w0, b0, c.prec)


def stats_of(d):
    return {s["name"]: s for s in d.kernel_stats(0)}


def same(got, want):
    return abs(got - want) <= 1e-9 * max(abs(want), 1.0)


def report(name, err, bar):
    print(f"INFER_EDGE {name} err {err:.3e} bar {bar:.1e} ratio {err / bar:.4f}")
    assert err < bar, (name, err, bar)


def bar_of(c, derived=False):
    return br.BF16_QTOL if c.prec else (ic.BAR_DERIVED if derived else ic.BAR_F32)


# ---------------------------------------------------------------------------------------------------------------- A, D: one forward call
def run_boards(xq, name, c):
    S = boards_of(xq, c.n, c.seed)
    d, net = handle_of(xq, c)
    env = xq.VecEnv(c.n)
    try:
        env.set_state(S)
        d.kernel_stats(2)
        q = d.q_boards(env, c.n_out).cpu().numpy().astype(np.float64)
        st = stats_of(d)
        head = "gemm_q90_select" if c.n_out <= 96 else "gemm_q_full"
        assert st["l0_forward_gather"]["launches"] == 1 and same(st["l0_forward_gather"]["bytes"], ic.l0_bytes(c, "gather")), st
        if len(c.sizes) > 3:
            assert st["gemm_hidden_fwd"]["launches"] == len(c.sizes) - 3 and same(st["gemm_hidden_fwd"]["flops"], ic.hidden_flops(c, False)), st
        assert st[head]["launches"] == 1 and same(st[head]["flops"], ic.head_flops(c, False)), st
        report(name, float(np.abs(q - br.q_rows(net, S, c.n_out)).max()), bar_of(c))
    finally:
        env.close(); d.close()


def run_ldq(xq, name, c):
    """a 90-output net the way make_player asks for it: n_out = 90 into rows of 96 floats; columns 90..95 must come back untouched"""
    import torch
    from cn_chess_ai_amd import _capi
    S = boards_of(xq, c.n, c.seed)
    d, net = handle_of(xq, c)
    env = xq.VecEnv(c.n)
    ldq = c.opt["ldq"]
    try:
        env.set_state(S)
        q = torch.full((c.n, ldq), -7.5, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _capi.call("xq_dqn_forward_boards_dev", d.handle, 0, C.c_void_p(env.boards_dev()), c.n, c.n_out, C.c_void_p(q.data_ptr()), ldq)
        _capi.call("xq_stream_synchronize", None)
        torch.cuda.synchronize()
        q = q.cpu().numpy().astype(np.float64)
        assert (q[:, c.n_out:] == -7.5).all(), "a column past n_out was written"
        report(name, float(np.abs(q[:, :c.n_out] - br.q_rows(net, S, c.n_out)).max()), bar_of(c))
    finally:
        env.close(); d.close()


# ---------------------------------------------------------------------------------------------------------------- B, D: the select chain
def check_select_stats(c, st, call):
    form = ic.sums_form(c, call)
    ride = ic.head_rides(c)
    g = st["l0_forward_gather"]
    assert g["launches"] == 1 and same(g["bytes"], ic.l0_bytes(c, form)), (call, form, g)
    if len(c.sizes) > 3:
        h = st["gemm_hidden_fwd"]
        assert h["launches"] == len(c.sizes) - 3 and same(h["flops"], ic.hidden_flops(c, ride)), (call, ride, h)
    q = st["gemm_q90_select"]
    assert q["launches"] == 1 and same(q["flops"], ic.head_flops(c, ride, 96)), (call, ride, q)
    return form


def run_select(xq, name, c):
    import torch
    from cn_chess_ai_amd import dist as xd
    S = boards_of(xq, c.n, c.seed)
    d, net = handle_of(xq, c)
    env = xq.VecEnv(c.n)
    worst = {"full": 0.0, "derived": 0.0}
    try:
        cur, nds = S, np.zeros(c.n, np.int64)
        env.set_state(cur)
        for call in range(1, 5):
            if call > 1 and c.opt.get("edit"):
                cur, nds = ic.edit_boards(cur, call, c.seed)
                assert set(nds) == set(ic.ND_CYCLE)
                env.set_state(cur)                               # in place: the same device pointer, the same n
            d.kernel_stats(2)
            q = d.select_q(env).cpu().numpy().astype(np.float64)
            form = check_select_stats(c, stats_of(d), call)
            err = np.abs(q - br.q_rows(net, cur, 96)).max(axis=1)
            from_kept = (nds <= 8) & (form == "derived")         # a row with more differences is summed in full again
            worst["derived"] = max(worst["derived"], float(err[from_kept].max(initial=0.0)))
            worst["full"] = max(worst["full"], float(err[~from_kept].max(initial=0.0)))
        if c.opt.get("drop"):                                    # a parameter update (of nothing) drops the kept sums
            ptr, n = d.grad_buffer()
            xd.wrap_device_floats(ptr, n).zero_()
            torch.cuda.synchronize()
            d.apply_grads(0.05, 1.0)
            w1, b1 = d.get_params()
            assert np.array_equal(w1, net.w) and np.array_equal(b1, net.b)
            d.kernel_stats(2)
            q5 = d.select_q(env).cpu().numpy()
            # the last period had four calls: the first of the next keeps its full sum (never derives)
            st = stats_of(d)
            assert same(st["l0_forward_gather"]["bytes"], ic.l0_bytes(c, "kept")), st["l0_forward_gather"]
            assert np.array_equal(q5, d.q_boards(env, 96).cpu().numpy())
            worst["full"] = max(worst["full"], float(np.abs(q5 - br.q_rows(net, cur, 96)).max()))
        if ic.sums_form(c, 3) == "derived":
            report(name + "[derived]", worst["derived"], bar_of(c, derived=True))
        report(name, worst["full"], bar_of(c))
    finally:
        env.close(); d.close()


# ---------------------------------------------------------------------------------------------------------------- C: the trainer's collect
def run_collect(xq, name, c):
    import torch
    n, versus, sfx = c.n, bool(c.opt.get("versus")), "@select" if c.opt["overlap"] else ""
    seed = 0x5EED + c.seed
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=c.sizes, learning_rate=0.01, gamma=0.99, epsilon=0.0, replay_capacity=4096, minibatch=n,
                           td_net=0, backprop_mode=1, target_sync_interval=0, seed=seed, first_game_id=0, overlap_collect=c.opt["overlap"])
    t = xq.Trainer(cfg)
    d, net = handle_of(xq, c)                                    # the composition's handle, and the parameters of both
    twin = xq.VecEnv(n, seed=seed, first_game_id=0)
    try:
        t.dqn.set_params(net.w, net.b)
        t.dqn.updateTargetNetwork()
        if versus:
            t.set_opponent("random")
        t.random_plies(25)
        S0, M0 = t.env.get_state()
        assert np.array_equal(S0, oracle_positions(n, 25, seed)[0])      # the positions of the CPU pre-check of the clear-best condition
        t.dqn.kernel_stats(2)
        t.collect()
        torch.cuda.synchronize()
        S1, _ = t.env.get_state()
        st = stats_of(t.dqn)
        ride = ic.head_rides(c)
        assert st["l0_forward_gather" + sfx]["launches"] == 1 and same(st["l0_forward_gather" + sfx]["bytes"], ic.l0_bytes(c, "gather")), st
        if len(c.sizes) > 3:
            assert same(st["gemm_hidden_fwd" + sfx]["flops"], ic.hidden_flops(c, ride)), st
        if ride:                                                 # the env kernel finishes the head itself
            assert "gemm_q90_select" + sfx not in st, st
        else:
            assert same(st["gemm_q90_select" + sfx]["flops"], ic.head_flops(c, False, 96)), st
        if not versus:
            assert st["env_selfplay_step"]["launches"] == 1
        ring = [t.replay.get(g) for g in range(n)]
        S = np.stack([r[0] for r in ring])                       # the boards the learner moved on
        A = np.array([r[1] for r in ring], np.int64)
        M = M0.copy()
        if versus:
            M[:, 1] = np.arange(n) & 1                           # the learner is Black in the odd games
        else:
            assert np.array_equal(S, S0)
        twin.set_state(S, M)
        codes, counts = twin.legal_moves()
        dests = [codes[g, :counts[g]].astype(np.int64) % 90 for g in range(n)]
        q = br.q_rows(net, S, 90)
        clear, bad = ic.move_checks(q, A, dests, ic.BAR_F32, idle_ok=versus)
        print(f"INFER_EDGE {name} clear {clear} of {n} failures {len(bad)}")
        assert not bad, bad[:5]
        assert clear >= 0.95 * n, clear
        if not versus:                                           # the bits of the composition: select_q, then the env step on the twin
            twin.set_state(S0, M0)
            qd = d.select_q(twin)
            twin.selfplay_step_dev(qd.data_ptr(), 96, 0.0)
            torch.cuda.synchronize()
            assert np.array_equal(twin.get_state()[0], S1)
            report(name, float(np.abs(qd.cpu().numpy()[:, :90] - q).max()), ic.BAR_F32)
    finally:
        t.close(); twin.close(); d.close()


# ---------------------------------------------------------------------------------------------------------------- E: the dense forward
def run_dense(xq, name, c):
    S = boards_of(xq, c.n, c.seed)
    d, net = handle_of(xq, c)
    try:
        x = br.one_hot(S)
        x[-32:] = np.random.default_rng(c.seed).uniform(-1, 1, size=(32, c.sizes[0]))
        d.kernel_stats(2)
        q = d.getQValues(x)
        st = stats_of(d)
        assert st["gemm_l0_dense_fwd"]["launches"] == 1 and same(st["gemm_l0_dense_fwd"]["flops"], 2.0 * c.n * c.sizes[1] * c.sizes[0]), st
        assert st["gemm_q_full"]["launches"] == 1 and same(st["gemm_q_full"]["flops"], ic.head_flops(c, False)), st
        assert q.shape == (c.n, c.n_out)
        report(name, float(np.abs(q - br.q_rows(net, x, c.n_out)).max()), bar_of(c))
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------------------------- F: the derived s' chain
def run_td(xq, name, c):
    k = tc._case("F", "-".join(str(s) for s in c.sizes), c.n, 0, c.prec, seed=c.seed)
    S = boards_of(xq, c.n, c.seed)
    S2, nds = ic.edit_boards(S, 0, c.seed)
    assert set(nds) == set(ic.ND_CYCLE)
    rng = np.random.default_rng(c.seed + 5)
    A = rng.integers(0, 90, c.n).astype(np.int32)
    R = rng.uniform(-0.5, 0.5, c.n).astype(np.float32)
    D = np.zeros(c.n, np.uint8)
    f = None
    for derive in (True, False):
        d = net_of(xq, k)
        try:
            if c.wscale != 1.0:
                w, b = d.get_params()
                w[br.offsets(c.sizes)[0][-1]:] *= c.wscale
                d.set_params(w, b)
            d.set_precision(c.prec)
            d.set_l0_derive(derive)
            w0, b0 = d.get_params()
            d.kernel_stats(2)
            q_dev, y_dev = d.td_update(S, S2, A, R, D, td_net=0, mode=k.mode, learning_rate=k.lr, grad_scale=k.scale)
            st = stats_of(d)
            assert st["l0_forward_gather"]["launches"] == 1, st
            new_w, new_b = d.get_params()
            if f is None:
                net = br.Net(c.sizes, w0, b0, c.prec)
                f = br.forward(net, S, S2, A, R, D, 0.99, 0, c.prec)
            flipped, y_use = br.check_q_y(f, q_dev, y_dev, c.prec)
            qtol = br.BF16_QTOL if c.prec else br.QTOL
            print(f"INFER_EDGE {name}[derive={int(derive)}] y err {float(np.abs(y_dev - f.y).max()):.3e} q err {float(np.abs(q_dev - f.q).max()):.3e} bar {qtol:.1e}")
            if derive:
                bk = br.backward(net, f, k.mode, c.prec, None, y=y_use, bf16_layers=tc.bf16_delta_layers(k))
                u = br.accumulate(net, f, bk, c.prec, bf16_layers=tc.bf16_grad_layers(k))
                ratios = br.check_update(net, u, f, new_w, new_b, k.lr, k.scale, c.prec)
                print(f"INFER_EDGE {name} update err/bound {max(ratios.values()):.4f}")
        finally:
            d.close()


RUN = dict(boards=run_boards, ldq=run_ldq, select=run_select, collect=run_collect, dense=run_dense, td=run_td)


@pytest.mark.parametrize("name", list(ic.CASES))
def test_inference_on_a_selection_boundary_matches_fp64(xq, name):
    c = ic.CASES[name]
    RUN[c.kind](xq, name, c)
