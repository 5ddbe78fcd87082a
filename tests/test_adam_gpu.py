"""The Adam optimizer of xq_dqn_apply_grads (xq_dqn_set_optimizer, adam_segments_kernel) on the device — `pytest -m gpu`.

Reference and bounds: tests/adam_ref.py (fp64 restatement of torch.optim.Adam's rule, the rounding bound of one device step from the
device's own read-back state, the bound that carries a gradient error through the step).  The gradient reference and its error budget
at full size are tests/batch_ref.py's, unchanged.

Largest err / bound observed on an MI355X: see profiles/NOTES.md ("Adam optimizer").
"""
import ctypes as C

import numpy as np
import pytest

import adam_ref as ar
import batch_ref as br
import xqoracle as xo
from test_dqn_gpu import CFG2_NET, REF_NET, make_net
from test_td_full_size_gpu import selfplay_batch

pytestmark = pytest.mark.gpu

MISALIGNED_NET = [1260, 127, 129, 8100]     # hidden product 127 x 129 and everything behind it: odd lengths, pointers off 16 bytes


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def state_ref(sizes, d):
    """(m_w, m_b, v_w, v_b, steps): the device's Adam state in the reference flat layout"""
    m, v, t = d.optimizer_state()
    mw, mb = ar.to_reference(sizes, m.astype(np.float64))
    vw, vb = ar.to_reference(sizes, v.astype(np.float64))
    return mw, mb, vw, vb, t


def same_bits(a, b):
    return np.array_equal(f32(a).view(np.uint32), f32(b).view(np.uint32))


# ---- 1. kernel against the reference, gradient injected ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET, MISALIGNED_NET], ids=["256x256_vec4", "128_vec4", "127x129_scalar"])
def test_kernel_matches_reference_with_injected_gradient(xq, sizes):
    """20 applies of a seeded gradient written straight into the gradient buffer.  After each one p, m and v lie within the one-step
    rounding bound of adam_ref started from the state read back before that step.  1260-256-256 and 1260-128: every segment takes the
    16-byte loop; 1260-127-129: layer 0 takes it, the 127 x 129 product, the output rows and both bias segments take the scalar loop."""
    import torch
    from cn_chess_ai_amd import dist as xd
    d, _, _ = make_net(xq, sizes, seed=31)
    d.set_optimizer("adam")
    assert d.optimizer() == dict(kind="adam", beta1=0.9, beta2=0.999, eps=1e-8, steps=0)
    ptr, n = d.grad_buffer()
    assert n == ar.layout(sizes)["n"]
    G = xd.wrap_device_floats(ptr, n)
    cw, cb = ar.covered(sizes)
    rng = np.random.default_rng(len(sizes) * 1000 + sizes[1])
    lr, gs = 1e-3, 1.0 / 3.0
    worst = dict(p=0.0, m=0.0, v=0.0)
    for t in range(1, 21):
        g = (10.0 ** rng.uniform(-12, 4, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
        g[rng.random(n) < 0.2] = 0.0
        g[rng.random(n) < 0.01] = np.float32(1e4) * rng.choice([-1.0, 1.0])
        sub = rng.random(n) < 0.02
        g[sub] = (rng.uniform(-1, 1, size=int(sub.sum())) * 1e-38).astype(np.float32)        # subnormal scale
        if t > 1:
            g[:n // 8] = -prev[:n // 8]                                                       # exact sign flips
        prev = g
        w0, b0 = d.get_params()
        mw, mb, vw, vb, steps = state_ref(sizes, d)
        assert steps == t - 1
        G.copy_(torch.from_numpy(g))
        torch.cuda.synchronize()
        d.apply_grads(lr, gs)
        w1, b1 = d.get_params()
        mw1, mb1, vw1, vb1, steps = state_ref(sizes, d)
        assert steps == t
        gw, gb = ar.to_reference(sizes, g.astype(np.float64))
        for p0, m0, v0, gg, p1, m1, v1, cov in ((w0, mw, vw, gw, w1, mw1, vw1, cw), (b0, mb, vb, gb, b1, mb1, vb1, cb)):
            (rp, rm, rv), (bp, bm, bv) = ar.one_step_bound(p0[cov], m0[cov], v0[cov], gg[cov], t, lr, gs)
            for k, got, ref, bound in (("p", p1[cov], rp, bp), ("m", m1[cov], rm, bm), ("v", v1[cov], rv, bv)):
                worst[k] = max(worst[k], float((np.abs(got - ref) / bound).max()))
            assert np.array_equal(p1[~cov], p0[~cov])                                         # what the buffer does not cover
    print("adam one-step err/bound", sizes, {k: round(x, 4) for k, x in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert worst["p"] > 0.01 and np.abs(w1 - w0).max() > 0
    d.close()


# ---- 2. the slab path has the bits of the buffer path -----------------------------------------------------------------------------
def ring(xq, batch, seed=0xABC):
    S, A, R, D, S2 = batch
    rp = xq.ReplayBuffer(len(S), seed=seed)
    rp.push(S, A, R, D, S2)
    return rp


@pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET], ids=["256x256", "128"])
def test_slab_path_has_the_bits_of_the_buffer_path(xq, sizes):
    """The same 8192-sample minibatches from a ring, once with xq_dqn_set_fused_apply(1) — the Adam kernel sums the partial-sum slabs
    itself — and once with 0, where one launch reduces them into the gradient buffer first: parameters, m and v bit-identical."""
    n = 8192
    batch = selfplay_batch(xq, n, seed=77, plies=25, every=9)
    got = []
    for fused in (1, 0):
        d, _, _ = make_net(xq, sizes, seed=5)
        d.set_optimizer("adam")
        d.set_fused_apply(fused)
        rp = ring(xq, batch)
        for _ in range(3):
            rp.sample(n)
            d.td_grads_replay(rp, n, td_net=0, mode=0)
            d.apply_grads(1e-3, 1.0 / n)
        got.append(d.get_params() + d.optimizer_state())
        rp.close(); d.close()
    (w1, b1, m1, v1, t1), (w0, b0, m0, v0, t0) = got
    assert t1 == t0 == 3
    assert np.array_equal(w1, w0) and np.array_equal(b1, b0)
    assert np.array_equal(m1.view(np.uint32), m0.view(np.uint32)) and np.array_equal(v1.view(np.uint32), v0.view(np.uint32))
    assert np.abs(m1).max() > 0 and np.abs(v1).max() > 0


# ---- 3. untouched stays untouched -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET], ids=["256x256", "128"])
def test_untouched_parameters_stay_untouched(xq, sizes):
    """Five TD steps on five different minibatches under Adam: rows >= 96 of W_out, the output rows and biases of actions never taken
    and the W0 columns of (square, piece) pairs on no board keep their bits, and their m and v are exactly 0 (no weight decay, no
    step without a gradient).  The screening shadow, which keeps rows >= 96 between steps, therefore still gives the full product's
    TD targets."""
    from cn_chess_ai_amd import _capi
    n = 2048
    d, w, b = make_net(xq, sizes, seed=13)
    d.set_optimizer("adam")
    d.set_qmax_mode(_capi.QMAX_SCREENED)
    w0, b0 = d.get_params()
    L, nl = sizes, len(sizes) - 1
    seen = np.zeros(L[0], bool)
    taken = np.zeros(L[-1], bool)
    batches = [selfplay_batch(xq, n, seed=300 + i, plies=10 + 7 * i, every=6 + i) for i in range(5)]
    for S, A, R, D, S2 in batches:
        d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=1e-3, grad_scale=1.0 / n)
        seen |= br.one_hot(S[A >= 0]).any(axis=0)
        taken[A[A >= 0]] = True
    w1, b1 = d.get_params()
    mw, mb, vw, vb, steps = state_ref(sizes, d)
    assert steps == 5
    H = L[-2]
    wo = len(w1) - L[-1] * H
    bo = len(b1) - L[-1]
    Wout0, Wout1 = w0[wo:].reshape(L[-1], H), w1[wo:].reshape(L[-1], H)
    assert np.array_equal(Wout1[96:], Wout0[96:])
    assert not taken[90:].any() and taken.any()
    assert np.array_equal(Wout1[~taken], Wout0[~taken]) and np.array_equal(b1[bo:][~taken], b0[bo:][~taken])
    assert not np.array_equal(Wout1[taken], Wout0[taken])
    W00, W01 = w0[:L[0] * L[1]].reshape(L[1], L[0]), w1[:L[0] * L[1]].reshape(L[1], L[0])
    assert (~seen).any() and np.array_equal(W01[:, ~seen], W00[:, ~seen]) and not np.array_equal(W01[:, seen], W00[:, seen])
    for s in (mw, vw):
        assert not s[:L[0] * L[1]].reshape(L[1], L[0])[:, ~seen].any()
        assert not s[wo:].reshape(L[-1], H)[~taken].any() and s[wo:].reshape(L[-1], H)[taken].any()
    for s in (mb, vb):
        assert not s[bo:][~taken].any() and s[bo:][taken].any()
    # the screened maximum on the trained parameters.  lr = 0 moves nothing (the step is -0 * m / den).  Two statements:
    # (1) it equals the full fp32 product in the sense of test_dqn_gpu.py (the same fp32 maxima up to the summation order of the
    #     candidate's dot product: < 2e-6);
    # (2) same y bits in both modes as a handle that receives the trained parameters through set_params, which converts the whole
    #     screening shadow afresh: the kept rows >= 96 of the trained handle's shadow are still the right ones.
    S, A, R, D, S2 = batches[0]
    e, _, _ = make_net(xq, sizes, seed=14)
    e.set_optimizer("adam")
    e.set_params(w1, b1)
    ys, ye = {}, {}
    for mode in (_capi.QMAX_FULL, _capi.QMAX_SCREENED):
        d.set_qmax_mode(mode); e.set_qmax_mode(mode)
        _, ys[mode] = d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=0.0, grad_scale=1.0 / n)
        _, ye[mode] = e.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=0.0, grad_scale=1.0 / n)
        assert np.array_equal(ys[mode].view(np.uint32), ye[mode].view(np.uint32)), mode
    w2, b2 = d.get_params()
    assert np.array_equal(w2, w1) and np.array_equal(b2, b1)
    diff = np.abs(ys[0].astype(np.float64) - ys[1])
    print("screened vs full y: max |diff|", float(diff.max()), "samples with other bits", int((ys[0].view(np.uint32) != ys[1].view(np.uint32)).sum()))
    assert diff.max() < 2e-6
    e.close()
    assert d.qmax_stats()[0] >= 1
    d.close()


# ---- 4. full size against fp64 ----------------------------------------------------------------------------------------------------
def flat_budget(net, u, scale, tol):
    """E = scale (tau T + eta U) of batch_ref.update_ratios per element, as flat (weights, biases) in the reference layout"""
    tau, eta = tol["tau"], tol["eta"]
    Ew, Eb = np.zeros_like(net.w), np.zeros_like(net.b)
    for l in range(net.nl):
        e = eta[l] if l < net.nl - 1 else eta[-1]
        L0, L1 = net.sizes[l], net.sizes[l + 1]
        U = u.U[l] if u.U[l].ndim == 2 else u.U[l][None, :]
        blk = Ew[net.wo[l]:net.wo[l] + L0 * L1].reshape(L1, L0)
        blk[:u.gW[l].shape[0]] = scale * (tau * u.T[l] + e * U)
        Eb[net.bo[l]:net.bo[l] + u.gB[l].shape[0]] = scale * (tau * u.TB[l] + e * u.UB[l])
    return Ew, Eb


def test_full_size_trainer_steps_against_fp64(xq):
    """Three TD steps at 8192 x 256^2 through the trainer as bench.py composes it (collect overlapped on its own stream, exact
    screening, layer 0 of s' derived, fused launches, slab sums inside the optimizer kernel), Adam on.  Before each step parameters and
    optimizer state are read back; the fp64 gradient of the re-derived minibatch and its per-element error budget E come from
    batch_ref (TOLERANCES unchanged); E goes through the step with adam_ref.gradient_error_bound, the step's own rounding through
    adam_ref.one_step_bound.  Every covered element of p, m and v is checked; every other parameter must keep its bits."""
    from cn_chess_ai_amd import _capi
    n, cap, lr, seed = 8192, 1 << 16, 1e-3, 0x5EED
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=CFG2_NET, learning_rate=lr, gamma=0.99, epsilon=0.1, replay_capacity=cap, minibatch=n,
                           td_net=_capi.TD_ONLINE_NET, backprop_mode=_capi.BACKPROP_REFERENCE, target_sync_interval=10, mean_gradient=1,
                           seed=seed, first_game_id=0, overlap_collect=1, collects_per_update=1)
    t = xq.Trainer(cfg)
    t.dqn.set_qmax_mode(_capi.QMAX_SCREENED)
    t.dqn.set_l0_derive(True)
    t.dqn.set_fused_apply(True)
    t.dqn.set_optimizer("adam")
    t.random_plies(300)
    for _ in range(cap // n):
        t.collect()
    sizes = CFG2_NET
    cw, cb = ar.covered(sizes)
    tol = br.TOLERANCES[br.PRECISION_F32]
    scale = 1.0 / n
    rseed = seed + 0x1234567
    key = (rseed & 0xFFFFFFFF, rseed >> 32)
    b1, b2 = ar.BETA1, ar.BETA2
    worst = dict(p=0.0, m=0.0, v=0.0)
    for k in range(3):
        w0, b0 = t.dqn.get_params()
        mw, mb, vw, vb, steps = state_ref(sizes, t.dqn)
        assert steps == k
        size, _, total = t.replay.stats()
        assert size == cap
        wpos = total % cap
        t.learn_grads()
        # minibatch k: sample call #k of the ring's Philox stream.  From the second iteration on it is drawn from the ring minus the n
        # slots this iteration's collect writes.  The first one finds the collects that filled the ring still counted as in flight
        # (nothing older than them exists): the trainer waits for them and draws from the whole ring, so its transitions are read back
        # here, before this iteration's collect overwrites the first n slots.
        start, count = ((wpos + n) % cap, cap - n) if k > 0 else (0, cap)
        slots = [(start + xo.philox((i, 0, k, 1), key)[0] % count) % cap for i in range(n)]
        trans = [t.replay.get(s) for s in slots]
        t.collect(); t.learn_apply(1)
        w1, b1_ = t.dqn.get_params()
        mw1, mb1, vw1, vb1, steps = state_ref(sizes, t.dqn)
        assert steps == k + 1
        qsa, y = t.dqn.last_td_values(n)
        S, A, R, D, S2 = (np.array([tr[j] for tr in trans]) for j in range(5))
        net = br.Net(sizes, w0, b0)
        f = br.forward(net, S, S2, A, R, D, 0.99, 0)
        br.check_q_y(f, qsa, y, br.PRECISION_F32)
        u = br.accumulate(net, f, br.backward(net, f, 0))
        gw, gb = br.flat_grads(net, u)
        Ew, Eb = flat_budget(net, u, scale, tol)
        tt = k + 1
        for p0, m0, v0, g, E, p1, m1, v1, cov in ((w0, mw, vw, gw, Ew, w1, mw1, vw1, cw), (b0, mb, vb, gb, Eb, b1_, mb1, vb1, cb)):
            assert np.array_equal(p1[~cov], p0[~cov])
            p0, m0, v0, g, E, p1, m1, v1 = (x[cov] for x in (p0, m0, v0, g, E, p1, m1, v1))
            (rp, rm, rv), (bp, bm, bv) = ar.one_step_bound(p0, m0, v0, g, tt, lr, scale)
            # the rounding bound at the far end of the gradient's interval as well (it grows with |g'| except through den)
            _, (bp2, bm2, bv2) = ar.one_step_bound(p0, m0, v0, np.abs(g) + E / scale, tt, lr, scale)
            bp, bm, bv = np.maximum(bp, bp2), np.maximum(bm, bm2), np.maximum(bv, bv2)
            gp = scale * g
            dS = ar.gradient_error_bound(m0, v0, gp, E, tt, lr)
            bound = dict(p=dS + bp, m=(1.0 - b1) * E + bm, v=(1.0 - b2) * (2.0 * np.abs(gp) * E + E * E) + bv)
            for name, got, ref in (("p", p1, rp), ("m", m1, rm), ("v", v1, rv)):
                r = np.abs(got - ref) / bound[name]
                worst[name] = max(worst[name], float(r.max()))
        print("adam full-size step", k + 1, "err/bound so far", {q: round(x, 4) for q, x in worst.items()})
        assert np.abs(w1 - w0).max() > 0
    assert max(worst.values()) <= 1.0, worst
    assert t.dqn.qmax_stats()[0] == 3
    t.close()


# ---- 5. bf16 net ------------------------------------------------------------------------------------------------------------------
def test_bf16_shadow_is_the_rounded_master(xq):
    """XQ_PRECISION_BF16, two Adam steps: the bf16 shadow the kernel refreshes equals bf16_round of the new fp32 master weights bit for
    bit.  The shadow is what the bf16 forward passes read: a second handle that gets the trained master weights through set_params
    (which converts every weight afresh) must then produce the same Q bits on every board, through every layer."""
    from cn_chess_ai_amd import _capi
    n = 2048
    for sizes in (CFG2_NET, REF_NET):
        d, _, _ = make_net(xq, sizes, seed=3)
        d.set_precision(_capi.PRECISION_BF16)
        d.set_optimizer("adam")
        w0, _ = d.get_params()
        for i in range(2):
            S, A, R, D, S2 = selfplay_batch(xq, n, seed=40 + i, plies=12 + i, every=8)
            d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=1e-3, grad_scale=1.0 / n)
        w1, b1 = d.get_params()
        assert d.optimizer()["steps"] == 2 and np.abs(w1 - w0).max() > 1e-4
        e, _, _ = make_net(xq, sizes, seed=4)
        e.set_precision(_capi.PRECISION_BF16)
        e.set_params(w1, b1)
        env = xq.VecEnv(n, seed=9)
        for _ in range(15):
            env.selfplay_step(None)
        qa, qb = d.q_boards(env, 96).cpu().numpy(), e.q_boards(env, 96).cpu().numpy()
        assert np.array_equal(qa.view(np.uint32), qb.view(np.uint32))
        # and the untrained weights give other bits: the comparison sees the shadow
        e.set_params(w0, b1)
        assert not np.array_equal(qa, e.q_boards(env, 96).cpu().numpy())
        env.close(); d.close(); e.close()


# ---- 6. communicator --------------------------------------------------------------------------------------------------------------
def test_one_rank_communicator_has_the_same_bits(xq):
    """Adam behind the all-reduce of a one-rank RCCL communicator: bit-identical to the same loop without one, 3 steps."""
    from cn_chess_ai_amd import dist as xd
    mk = lambda: xq.TrainerConfig(n_games=512, layer_sizes=(1260, 64, 64, 8100), replay_capacity=4096, minibatch=1024, td_net=0,
                                  target_sync_interval=3, seed=99, overlap_collect=1)
    ta, tb = xq.Trainer(mk()), xq.Trainer(mk())
    comm = xd.Comm(rank=0, world=1)
    tb.set_comm(comm)
    for t in (ta, tb):
        t.dqn.set_optimizer("adam")
        for _ in range(3):
            t.learn_grads(); t.collect(); t.learn_apply(1)
    assert comm.info()["collectives"] == 3
    (wa, ba), (wb, bb) = ta.dqn.get_params(), tb.dqn.get_params()
    ma, va, sa = ta.dqn.optimizer_state()
    mb, vb, sb = tb.dqn.optimizer_state()
    assert sa == sb == 3 and np.array_equal(wa, wb) and np.array_equal(ba, bb)
    assert np.array_equal(ma.view(np.uint32), mb.view(np.uint32)) and np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    assert np.array_equal(ta.env.get_state()[0], tb.env.get_state()[0])
    ta.close(); tb.close(); comm.close()


def test_doubled_gradient_with_world_size_two(xq):
    """"Sum over two identical ranks": the gradient buffer doubled in place, learn_apply(world_size=2).  Adam is invariant to the scale
    of g' only up to eps, and the scale goes into g' (not into the step), so the update is the single-rank one within the one-step
    bound, not by construction bit for bit."""
    import torch
    from cn_chess_ai_amd import dist as xd
    sizes = (1260, 128, 8100)
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    cfg = xq.TrainerConfig(n_games=256, layer_sizes=sizes, replay_capacity=0, minibatch=256, td_net=0)
    outs = []
    for world in (2, 1):
        t = xq.Trainer(cfg, stream=C.c_void_p(s.cuda_stream))
        t.dqn.set_optimizer("adam")
        ptr, n = t.dqn.grad_buffer()
        g = xd.wrap_device_floats(ptr, n)
        w0, b0 = t.dqn.get_params()
        t.collect(); t.learn_grads()
        torch.cuda.synchronize()
        g1 = g.cpu().numpy().copy()
        if world == 2:
            g.mul_(2.0)
            torch.cuda.synchronize()
        t.learn_apply(world_size=world)
        outs.append((w0, b0, g1) + t.dqn.get_params())
        t.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    (w0, b0, g2, w2, b2), (w0_, b0_, g1, w1, b1) = outs
    assert np.array_equal(w0, w0_) and np.array_equal(g1, g2) and np.abs(g1).max() > 0
    gw, gb = ar.to_reference(sizes, g1.astype(np.float64))
    cw, cb = ar.covered(sizes)
    for p0, g, pa, pb, cov in ((w0, gw, w1, w2, cw), (b0, gb, b1, b2, cb)):
        z = np.zeros(int(cov.sum()))
        (rp, _, _), (bp, _, _) = ar.one_step_bound(p0[cov], z, z, g[cov], 1, cfg.learning_rate, 1.0 / 256)
        assert (np.abs(pa[cov] - rp) <= bp).all() and (np.abs(pb[cov] - rp) <= bp).all()
        assert np.array_equal(pa[~cov], p0[~cov]) and np.array_equal(pb[~cov], p0[~cov])
    assert not np.array_equal(w1, w0)


# ---- 7. state API -----------------------------------------------------------------------------------------------------------------
def test_state_api_resume_reset_switch_and_errors(xq):
    from cn_chess_ai_amd import _capi
    sizes, n = CFG2_NET, 1024
    batches = [selfplay_batch(xq, n, seed=500 + i, plies=9 + 3 * i, every=7) for i in range(6)]

    def steps(d, which, lr=1e-3):
        for i in which:
            S, A, R, D, S2 = batches[i]
            d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=lr, grad_scale=1.0 / n)

    a, _, _ = make_net(xq, sizes, seed=2)
    a.set_optimizer("adam", beta1=0.8, beta2=0.99, eps=1e-6)
    assert a.optimizer() == dict(kind="adam", beta1=0.8, beta2=0.99, eps=1e-6, steps=0)
    steps(a, range(3))
    m, v, t = a.optimizer_state()
    assert t == 3 and m.dtype == np.float32 and len(m) == len(v) == a.grad_buffer()[1] and np.abs(m).max() > 0 and v.min() >= 0
    w, b = a.get_params()
    # set_params / load_model / update_target leave the state alone
    a.set_params(w, b); a.updateTargetNetwork()
    m_, v_, t_ = a.optimizer_state()
    assert t_ == 3 and np.array_equal(m_, m) and np.array_equal(v_, v)
    # resume on a new handle
    c, _, _ = make_net(xq, sizes, seed=77)
    c.set_optimizer("adam", beta1=0.8, beta2=0.99, eps=1e-6)
    c.set_params(w, b)
    c.set_optimizer_state(m, v, t)
    steps(a, range(3, 6)); steps(c, range(3, 6))
    assert all(np.array_equal(x, y) for x, y in zip(a.get_params() + a.optimizer_state()[:2], c.get_params() + c.optimizer_state()[:2]))
    assert a.optimizer_state()[2] == c.optimizer_state()[2] == 6
    # reset
    a.reset_optimizer()
    m0, v0, t0 = a.optimizer_state()
    assert t0 == 0 and not m0.any() and not v0.any() and a.optimizer()["kind"] == "adam" and a.optimizer()["beta1"] == 0.8
    # a call that keeps the kind keeps the state; changing the kind zeroes it
    steps(a, [0])
    a.set_optimizer("adam")
    assert a.optimizer_state()[2] == 1 and a.optimizer()["beta1"] == 0.9
    a.set_optimizer("sgd"); a.set_optimizer("adam")
    m0, v0, t0 = a.optimizer_state()
    assert t0 == 0 and not m0.any() and not v0.any()
    # SGD -> Adam -> SGD: SGD's bits are those of a handle that never switched
    p, _, _ = make_net(xq, sizes, seed=2)
    q, _, _ = make_net(xq, sizes, seed=2)
    q.set_optimizer("adam"); steps(q, [0]); q.set_optimizer("sgd")
    q.set_params(*p.get_params())
    steps(p, range(3), lr=0.05); steps(q, range(3), lr=0.05)
    assert all(np.array_equal(x, y) for x, y in zip(p.get_params(), q.get_params()))
    # backpropagate stays plain SGD and does not touch the state
    q.set_optimizer("adam"); steps(q, [1])
    mq, vq, tq = q.optimizer_state()
    x = br.one_hot(batches[0][0][:4])
    tgt = np.zeros((4, 8100))
    p.set_params(*q.get_params())
    p.backpropagate(x, tgt, 0.01, 1.0, _capi.BACKPROP_TEXTBOOK); q.backpropagate(x, tgt, 0.01, 1.0, _capi.BACKPROP_TEXTBOOK)
    assert all(np.array_equal(x_, y_) for x_, y_ in zip(p.get_params(), q.get_params()))
    mq2, vq2, tq2 = q.optimizer_state()
    assert tq2 == tq and np.array_equal(mq, mq2) and np.array_equal(vq, vq2)
    # error paths
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.5), dict(eps=-1e-9)):
        with pytest.raises(xq.XqError) as e:
            q.set_optimizer("adam", **bad)
        assert e.value.code == 1
    with pytest.raises(xq.XqError) as e:
        _capi.call("xq_dqn_set_optimizer", q.handle, 7, 0.0, 0.0, 0.0)
    assert e.value.code == 1
    for call in (lambda: p.optimizer_state(), lambda: p.set_optimizer_state(mq, vq, 1)):        # p is SGD
        with pytest.raises(xq.XqError) as e:
            call()
        assert e.value.code == 2
    assert p.optimizer() == dict(kind="sgd", beta1=0.9, beta2=0.999, eps=1e-8, steps=0)
    # refused while a TD step waits for its apply (as set_fused_apply)
    q.set_fused_apply(True)
    rp = ring(xq, batches[0])
    rp.sample(n)
    q.td_grads_replay(rp, n, td_net=0, mode=0)
    for call in (lambda: q.set_optimizer("sgd"), lambda: q.set_optimizer_state(mq, vq, 1)):
        with pytest.raises(xq.XqError) as e:
            call()
        assert e.value.code == 2 and "waiting" in str(e.value)
    q.apply_grads(1e-3, 1.0 / n)
    q.set_optimizer("sgd")
    for h in (a, c, p, q):
        h.close()
    rp.close()


# ---- 8. the default is untouched --------------------------------------------------------------------------------------------------
def test_default_is_sgd_with_the_same_bits_and_kernels(xq):
    """No set_optimizer call: the kernel statistics list sgd_apply and no adam_apply, and a 5-step trainer run has the bits of the same
    run on a handle where set_optimizer("sgd") was called.  With Adam the statistics list adam_apply and no sgd_apply."""
    mk = lambda: xq.TrainerConfig(n_games=1024, layer_sizes=CFG2_NET, replay_capacity=8192, minibatch=1024, td_net=0,
                                  target_sync_interval=3, seed=5, overlap_collect=1)
    outs, names = [], []
    for opt in (None, "sgd", "adam"):
        t = xq.Trainer(mk())
        if opt:
            t.dqn.set_optimizer(opt)
        t.dqn.kernel_stats(2)
        t.step(5)
        st = {s["name"]: s for s in t.dqn.kernel_stats(0)}
        names.append(st)
        outs.append(t.dqn.get_params() + (t.env.get_state()[0],))
        t.close()
    assert "sgd_apply" in names[0] and "adam_apply" not in names[0] and names[0]["sgd_apply"]["launches"] == 5
    assert set(names[0]) == set(names[1]) and {k: s["launches"] for k, s in names[0].items()} == {k: s["launches"] for k, s in names[1].items()}
    assert "adam_apply" in names[2] and "sgd_apply" not in names[2] and names[2]["adam_apply"]["launches"] == 5
    assert names[2]["adam_apply"]["exact"] == 5
    assert set(names[2]) - {"adam_apply"} == set(names[0]) - {"sgd_apply"}
    assert all(np.array_equal(x, y) for x, y in zip(outs[0], outs[1]))
    assert not np.array_equal(outs[0][0], outs[2][0])


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------
def test_facade_sets_the_optimizer_and_trains_with_it(xq):
    """xq::ChessAI::setOptimizer forwards to its network (xq::DQN::optimizer reads it back, defaults filled in, a beta of 1 is
    std::invalid_argument), and the batched train() takes the network's choice: under Adam no weight moves further than
    updates * lr / (1 - beta1) (|m| / sqrt(v) is at most 1 / sqrt(1 - beta2) per step only in theory; 10 x lr per update is generous),
    under SGD with the reference's rewards the same run moves them by other amounts."""
    import json
    import subprocess
    from test_adam_ref_cpu import build_adam_facade_probe
    exe = build_adam_facade_probe()
    out = subprocess.run([exe, "256", "300", "7"], check=True, capture_output=True, text=True, timeout=600).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["kind"], r["beta1"], r["beta2"], r["eps"], r["steps"]) == (1, 0.8, 0.99, 1e-6, 0)
    assert (r["default_beta1"], r["default_beta2"], r["default_eps"]) == (0.9, 0.999, 1e-8)
    assert r["refused"] == 1 and r["kind_after_sgd"] == 0
    assert r["adam_updates"] > 0 and r["sgd_updates"] > 0
    assert 0 < r["adam_max_dw"] <= r["adam_updates"] * 0.001 * 10
    assert r["sgd_max_dw"] > 0 and r["sgd_max_dw"] != r["adam_max_dw"]
