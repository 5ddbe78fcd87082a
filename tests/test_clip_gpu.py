"""Gradient clipping of xq_dqn_apply_grads (xq_dqn_set_grad_clip, grad_norm_kernel, the clip variants of the two apply kernels) on the
device — `pytest -m gpu`.

Reference and bounds: tests/clip_ref.py (fp64 restatement of torch.nn.utils.clip_grad_norm_ in front of SGD / Adam, the rounding bound of
one device step).  The gradient reference and its error budget end to end are tests/batch_ref.py's, unchanged.

Largest err / bound observed on an MI355X: see profiles/NOTES.md ("Gradient clipping").
"""
import ctypes as C
import math

import numpy as np
import pytest

import adam_ref as ar
import batch_ref as br
import clip_ref as cr
from test_adam_gpu import MISALIGNED_NET, flat_budget, ring, state_ref
from test_dqn_gpu import CFG2_NET, REF_NET, make_net
from test_td_full_size_gpu import selfplay_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


_BATCHES = {}


def batch(xq, n, seed):
    """selfplay_batch, computed once per (n, seed) and shared (never modified)"""
    if (n, seed) not in _BATCHES:
        _BATCHES[(n, seed)] = selfplay_batch(xq, n, seed=seed, plies=11 + seed % 17, every=7)
    return _BATCHES[(n, seed)]


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def snapshot(d, adam):
    out = list(d.get_params())
    if adam:
        out += list(d.optimizer_state()[:2])
    return out


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. norm, coefficient and the step, gradient injected -------------------------------------------------------------------------
def seeded_gradient(rng, n, kind):
    if kind == "zero":
        return np.zeros(n, np.float32)
    g = (10.0 ** rng.uniform(-12, 4, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    g[rng.random(n) < 0.2] = 0.0
    a = n // 3
    g[a:a + 4096] = (rng.uniform(-1, 1, size=4096) * 1e-38).astype(np.float32)               # a subnormal-scale slice
    if kind == "huge":
        g[rng.choice(n, size=5, replace=False)] = np.float32(1e15) * rng.choice([-1.0, 1.0], size=5)
    return g


def check_norm_and_coef(st, g, gs, max_norm):
    """last_norm against the exactly rounded fp64 norm to n 2^-52; last_coef == float32(c), or one ulp off where the norm lies within
    that distance of a rounding boundary of c.  Returns the fp64 coefficient."""
    n = g.size
    nrm = cr.norm(g, gs)
    tol = n * 2.0 ** -52
    assert abs(st["last_norm"] - nrm) <= tol * nrm, (st["last_norm"], nrm)
    c = cr.coef_of_norm(nrm, max_norm)
    c32 = np.float32(c)
    lo, hi = np.float32(cr.coef_of_norm(nrm * (1 + tol), max_norm)), np.float32(cr.coef_of_norm(nrm * (1 - tol), max_norm))
    dev = np.float32(st["last_coef"])
    assert float(dev) == st["last_coef"]
    assert dev == c32 or (lo != hi and abs(float(dev) - float(c32)) <= float(np.spacing(c32))), (dev, c32, lo, hi)
    return c


@pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET, MISALIGNED_NET], ids=["256x256_vec4", "128_vec4", "127x129_scalar"])
def test_norm_coefficient_and_step_with_injected_gradient(xq, sizes):
    """Seeded gradients written straight into the gradient buffer (magnitudes 1e-12 .. 1e4, a fifth exact zeros, a subnormal slice; one
    variant with five +-1e15 entries, one all zero), applied under SGD and under Adam with a max_norm that clips and one that does
    not.  Norm and coefficient against numpy fp64, every parameter (Adam: m and v too) inside clip_ref's one-step bound, what the
    buffer does not cover keeps its bits, the counters count.  1260-127-129: every segment but layer 0 takes the scalar loops."""
    import torch
    from cn_chess_ai_amd import dist as xd
    d, _, _ = make_net(xq, sizes, seed=31)
    ptr, n = d.grad_buffer()
    assert n == ar.layout(sizes)["n"]
    G = xd.wrap_device_floats(ptr, n)
    cw, cb = ar.covered(sizes)
    rng = np.random.default_rng(len(sizes) * 1000 + sizes[1])
    lr, gs = 1e-3, 1.0 / 3.0
    # (kind of gradient, max_norm as a multiple of the norm or absolute)
    plan = [("spread", ("rel", 0.25)), ("spread", ("rel", 4.0)), ("huge", ("abs", 1.0)), ("zero", ("abs", 1.0)), ("spread", ("abs", math.inf))]
    applies = clipped = 0
    worst = dict(sgd=0.0, p=0.0, m=0.0, v=0.0)
    d.set_grad_clip(1.0)
    assert d.grad_clip() == 1.0 and d.grad_clip_stats() == dict(last_norm=0.0, last_coef=0.0, applies=0, clipped=0)
    for opt in ("sgd", "adam"):
        d.set_optimizer(opt)
        for kind, (how, x) in plan:
            g = seeded_gradient(rng, n, kind)
            max_norm = x * cr.norm(g, gs) if how == "rel" else x
            d.set_grad_clip(max_norm)
            w0, b0 = d.get_params()
            if opt == "adam":
                mw, mb, vw, vb, steps = state_ref(sizes, d)
            G.copy_(torch.from_numpy(g))
            torch.cuda.synchronize()
            d.apply_grads(lr, gs)
            st = d.grad_clip_stats()
            c = check_norm_and_coef(st, g, gs, max_norm)
            applies += 1
            clipped += c < 1.0
            assert (st["applies"], st["clipped"]) == (applies, clipped)
            if kind == "zero" or x == math.inf or (how, x) == ("rel", 4.0):
                assert st["last_coef"] == 1.0
            else:
                assert st["last_coef"] < 1.0
            w1, b1 = d.get_params()
            gw, gb = ar.to_reference(sizes, g.astype(np.float64))
            if opt == "sgd":
                for p0, gg, p1, cov in ((w0, gw, w1, cw), (b0, gb, b1, cb)):
                    ref, bound = cr.sgd_one_step_bound(p0[cov], gg[cov], lr, gs, c)
                    worst["sgd"] = max(worst["sgd"], float((np.abs(p1[cov] - ref) / bound).max()))
                    assert np.array_equal(p1[~cov], p0[~cov])
            else:
                mw1, mb1, vw1, vb1, steps1 = state_ref(sizes, d)
                assert steps1 == steps + 1
                for p0, m0, v0, gg, p1, m1, v1, cov in ((w0, mw, vw, gw, w1, mw1, vw1, cw), (b0, mb, vb, gb, b1, mb1, vb1, cb)):
                    (rp, rm, rv), (bp, bm, bv) = cr.adam_one_step_bound(p0[cov], m0[cov], v0[cov], gg[cov], steps1, lr, gs, c)
                    for k, got, ref, bound in (("p", p1[cov], rp, bp), ("m", m1[cov], rm, bm), ("v", v1[cov], rv, bv)):
                        worst[k] = max(worst[k], float((np.abs(got - ref) / bound).max()))
                    assert np.array_equal(p1[~cov], p0[~cov])
            if kind == "zero" and opt == "sgd":
                assert np.array_equal(w1, w0) and np.array_equal(b1, b0)                     # a gradient of 0 stays 0 (Adam: m still moves p)
    print("clip one-step err/bound", sizes, {k: round(x, 4) for k, x in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    assert worst["sgd"] > 0.01 and worst["p"] > 0.01
    assert (applies, clipped) == (10, 4)
    d.close()


# ---- 2. not clipping is free of side effects --------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_not_clipping_has_the_bits_and_launches_of_off(xq, opt):
    """The same three TD steps from a ring with clipping off, with +inf and with a max_norm above every norm: parameters (and Adam's m
    and v) bit-identical.  Off: no grad_norm bracket, and the launch names and counts of a handle that was switched on and off again
    are those of one that was never asked; on: grad_norm once per apply in front of the same launches."""
    n = 1024
    S = batch(xq, n, 61)
    outs, stats, norms = [], [], []
    for mode in ("never", math.inf, 1e30, "on_then_off"):
        d, _, _ = make_net(xq, CFG2_NET, seed=5)
        d.set_optimizer(opt)
        if mode == "on_then_off":
            d.set_grad_clip(0.5); d.set_grad_clip(0.0)
        elif mode != "never":
            d.set_grad_clip(mode)
        assert d.grad_clip() == (0.0 if isinstance(mode, str) else mode)
        rp = ring(xq, S)
        d.kernel_stats(2)
        for _ in range(3):
            rp.sample(n)
            d.td_grads_replay(rp, n, td_net=0, mode=0)
            d.apply_grads(1e-2, 1.0 / n)
        stats.append({s["name"]: s["launches"] for s in d.kernel_stats(0)})
        outs.append(snapshot(d, opt == "adam"))
        if not isinstance(mode, str):
            st = d.grad_clip_stats()
            assert (st["applies"], st["clipped"], st["last_coef"]) == (3, 0, 1.0) and 0 < st["last_norm"] < 1e30
            norms.append(st["last_norm"])
        rp.close(); d.close()
    assert same(outs[0], outs[1]) and same(outs[0], outs[2]) and same(outs[0], outs[3])
    assert norms[0] == norms[1]
    apply = "adam_apply" if opt == "adam" else "sgd_apply"
    assert "grad_norm" not in stats[0] and stats[0][apply] == 3
    assert stats[3] == stats[0]
    for on in (stats[1], stats[2]):
        assert on["grad_norm"] == 3 and {k: v for k, v in on.items() if k != "grad_norm"} == stats[0]


@pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET, MISALIGNED_NET], ids=["256x256_vec4", "128_vec4", "127x129_scalar"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_clip_kernels_at_c_equal_one_have_the_bits_of_the_unclipped_kernels(xq, sizes, opt):
    """The clip variants of the apply kernels repeat the direct-gradient loops of the unclipped ones; with c == 1 they must give the same
    bits in the 16-byte loops and in the scalar loops (1260-127-129: every segment but layer 0).  Three injected gradients, applied with
    clipping off, with +inf and with a max_norm above the norm: parameters (Adam: m and v) bit-identical."""
    import torch
    from cn_chess_ai_amd import dist as xd
    n = ar.layout(sizes)["n"]
    rng = np.random.default_rng(sizes[1])
    gs = [seeded_gradient(rng, n, "spread") for _ in range(3)]
    outs = []
    for max_norm in (0.0, math.inf, 1e30):
        d, _, _ = make_net(xq, sizes, seed=31)
        d.set_optimizer(opt)
        d.set_grad_clip(max_norm)
        ptr, k = d.grad_buffer()
        G = xd.wrap_device_floats(ptr, k)
        w_init = d.get_params()[0]
        for g in gs:
            G.copy_(torch.from_numpy(g))
            torch.cuda.synchronize()
            d.apply_grads(1e-3, 1.0 / 3.0)
        if max_norm:
            st = d.grad_clip_stats()
            assert (st["applies"], st["clipped"], st["last_coef"]) == (3, 0, 1.0)
        outs.append(snapshot(d, opt == "adam"))
        d.close()
    assert same(outs[0], outs[1]) and same(outs[0], outs[2])
    assert not np.array_equal(outs[0][0], w_init)


# ---- 3. the slab path has the bits of the buffer path -----------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,opt", [(CFG2_NET, "sgd"), (CFG2_NET, "adam"), (REF_NET, "sgd")], ids=["256x256_sgd", "256x256_adam", "128_sgd"])
def test_slab_path_has_the_bits_of_the_buffer_path(xq, sizes, opt):
    """8192-sample minibatches (the smallest batch whose layer-0 gradient comes in more than one 1024-sample slab), clipping active:
    once with xq_dqn_set_fused_apply(1), where grad_norm_kernel sums the slabs itself, once with 0, where one launch reduces them
    first.  Norm, coefficient, parameters and Adam's state bit-identical after each of three steps, and the gradient buffer of the
    fused handle ends up holding the slab sums (the whole buffer equals the reduce-first handle's)."""
    import torch
    from cn_chess_ai_amd import dist as xd
    n = 8192
    S = batch(xq, n, 77)
    got = []
    for fused in (1, 0):
        d, _, _ = make_net(xq, sizes, seed=5)
        d.set_optimizer(opt)
        d.set_fused_apply(fused)
        d.set_grad_clip(2e-3)
        rp = ring(xq, S)
        seq = []
        for _ in range(3):
            rp.sample(n)
            d.td_grads_replay(rp, n, td_net=0, mode=0)
            d.apply_grads(1e-2, 1.0 / n)
            seq.append(d.grad_clip_stats())
        ptr, k = d.grad_buffer()
        torch.cuda.synchronize()
        buf = xd.wrap_device_floats(ptr, k).cpu().numpy().copy()
        got.append((seq, snapshot(d, opt == "adam"), buf))
        rp.close(); d.close()
    (seq1, p1, g1), (seq0, p0, g0) = got
    print("slab/buffer norms", [s["last_norm"] for s in seq1], "coefs", [s["last_coef"] for s in seq1])
    assert seq1 == seq0 and seq1[-1]["applies"] == 3
    assert any(s["last_coef"] < 1.0 for s in seq1) and seq1[-1]["clipped"] >= 1
    assert same(p1, p0)
    assert np.array_equal(bits(g1), bits(g0))
    L0 = sizes[0] * sizes[1]
    assert np.abs(g1[:L0]).max() > 0
    # the layer-0 segment is the gradient whose norm was reported
    assert abs(cr.norm(g1, 1.0 / n) - seq1[-1]["last_norm"]) <= k * 2.0 ** -52 * seq1[-1]["last_norm"]


SCALAR_TD_NET = [1260, 127, 129, 132, 8100]


@pytest.mark.parametrize("max_norm", [0.0, 1e-3], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_scalar_slab_loops_have_the_bits_of_the_buffer_path(xq, opt, max_norm):
    """No other fused-against-reduce-first test takes the scalar slab loops of the SGD, Adam and norm kernels: their nets have 16-byte
    aligned segments throughout.  1260-127-129-132-8100: the first hidden segment has 16383 elements and every segment behind it starts
    at an odd offset of the gradient buffer (176403, 193431, 206103, 206199), so all of them go through the scalar loops while layer 0
    takes the 16-byte loop.  (1260-127-129-8100, MISALIGNED_NET, has the same offsets but cannot take a TD step: the output-gradient
    kernel wants a last hidden width that is a multiple of 4, and with two hidden layers such a width puts every offset back on a
    multiple of 4.  Hence a third hidden layer, and the textbook backward rule, since the reference's is undefined where a layer
    widens.)  n = 1300: layer 0 in 2 slabs (the leftover loop alone), the output rows in 6 (one group of four, two leftovers), the bias
    column sums in 20 (five groups of four).  Two TD steps with xq_dqn_set_fused_apply(1) and with 0: parameters (Adam: m and v)
    bit-identical; clipping: norm, coefficient and the whole gradient buffer too.  The fused leg launched no reduce_slabs bracket and
    the other one did, so the slabs really were pending."""
    import torch
    from cn_chess_ai_amd import dist as xd
    sizes = SCALAR_TD_NET
    lay = ar.layout(sizes)
    assert (lay["wh"][1], lay["wh"][2], lay["wout"], lay["bout"], lay["bh"]) == (160020, 176403, 193431, 206103, 206199)
    assert sizes[1] * sizes[2] == 16383
    n = 1300
    S = batch(xq, n, 83)
    got = []
    for fused in (1, 0):
        d, _, _ = make_net(xq, sizes, seed=5)
        d.set_optimizer(opt)
        d.set_fused_apply(fused)
        d.set_grad_clip(max_norm)
        w_init = d.get_params()[0]
        rp = ring(xq, S)
        d.kernel_stats(2)
        seq = []
        for _ in range(2):
            rp.sample(n)
            d.td_grads_replay(rp, n, td_net=0, mode=1)
            d.apply_grads(1e-2, 1.0 / n)
            seq.append(d.grad_clip_stats() if max_norm else None)
        launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
        ptr, k = d.grad_buffer()
        torch.cuda.synchronize()
        buf = xd.wrap_device_floats(ptr, k).cpu().numpy().copy()
        got.append((seq, snapshot(d, opt == "adam"), buf, launches))
        rp.close(); d.close()
    (seq1, p1, g1, l1), (seq0, p0, g0, l0) = got
    print("scalar slab loops", opt, max_norm, seq1, {k: v for k, v in l0.items() if k not in l1 or l1[k] != v})
    assert "reduce_slabs" not in l1 and l0["reduce_slabs"] >= 2
    assert same(p1, p0)
    assert not np.array_equal(p1[0], w_init)
    if max_norm:
        assert seq1 == seq0 and seq1[-1]["applies"] == 2
        assert all(s["last_coef"] < 1.0 for s in seq1)
        assert np.array_equal(bits(g1), bits(g0))


# ---- 4. against fp64 end to end ---------------------------------------------------------------------------------------------------
def test_td_step_against_fp64_end_to_end(xq):
    """One TD step of 1024 self-play samples on 1260-256-256-8100 with clipping at half the reference's norm.  Gradient reference:
    batch_ref (td_step, flat_grads), coefficient derived from it in fp64.  The device norm lies within the gradient budget batch_ref
    grants (| ||a|| - ||b|| | <= ||a - b|| <= ||E||, E the per-element budget at the step's gradient scale), the parameters within its
    update budget with lr c in place of lr."""
    sizes, n, lr = CFG2_NET, 1024, 1.0
    gs = 16.0 / n
    S, A, R, D, S2 = batch(xq, n, 2024)
    d, _, _ = make_net(xq, sizes, seed=21)
    w0, b0 = d.get_params()
    net, f, bk, u = br.td_step(sizes, w0, b0, S, S2, A, R, D)
    gw, gb = br.flat_grads(net, u)
    nrm0 = gs * math.sqrt(float(np.sum(gw * gw) + np.sum(gb * gb)))
    max_norm = 0.5 * nrm0
    d.set_grad_clip(max_norm)
    q_dev, y_dev = d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=lr, grad_scale=gs)
    st = d.grad_clip_stats()
    w1, b1 = d.get_params()
    d.close()
    _, y_use = br.check_q_y(f, q_dev, y_dev, br.PRECISION_F32)
    u = br.accumulate(net, f, br.backward(net, f, 0, br.PRECISION_F32, None, y=y_use))
    gw, gb = br.flat_grads(net, u)
    nrm = gs * math.sqrt(float(np.sum(gw * gw) + np.sum(gb * gb)))
    Ew, Eb = flat_budget(net, u, gs, br.TOLERANCES[br.PRECISION_F32])
    budget = math.sqrt(float(np.sum(Ew * Ew) + np.sum(Eb * Eb))) + (len(gw) + len(gb)) * 2.0 ** -52 * nrm
    c = cr.coef_of_norm(nrm, max_norm)
    print("end to end: norm", st["last_norm"], "ref", nrm, "|diff| / budget", abs(st["last_norm"] - nrm) / budget,
          "coef", st["last_coef"], "ref", c)
    assert abs(st["last_norm"] - nrm) <= budget
    assert 0.4 < c < 0.6 and st["clipped"] == 1 and abs(st["last_coef"] - c) <= c * (budget / nrm + 2.0 ** -23)
    ratios = br.check_update(net, u, f, w1, b1, lr * c, gs, br.PRECISION_F32)
    print("end to end: err/bound", {k: round(v, 4) for k, v in ratios.items()})
    assert np.abs(w1 - w0).max() > 0


# ---- 5. reach ---------------------------------------------------------------------------------------------------------------------
def test_bf16_shadow_is_the_rounded_master_and_rows_from_96_keep_their_bits(xq):
    """XQ_PRECISION_BF16, two clipped SGD steps: a second handle that gets the trained master weights through set_params (which converts
    every weight afresh) produces the same Q bits on every board, so the shadow the clip kernel refreshed is the rounded master; rows
    >= 96 of W_out and their biases keep their bits."""
    from cn_chess_ai_amd import _capi
    n, sizes = 2048, REF_NET
    d, _, _ = make_net(xq, sizes, seed=3)
    d.set_precision(_capi.PRECISION_BF16)
    d.set_grad_clip(1e-3)
    w0, b0 = d.get_params()
    for i in range(2):
        S, A, R, D, S2 = batch(xq, n, 40 + i)
        d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=0.5, grad_scale=1.0 / n)
    st = d.grad_clip_stats()
    assert st["applies"] == 2 and st["clipped"] == 2
    w1, b1 = d.get_params()
    assert np.abs(w1 - w0).max() > 1e-5
    H, NO = sizes[-2], sizes[-1]
    wo, bo = len(w1) - NO * H, len(b1) - NO
    assert np.array_equal(w1[wo:].reshape(NO, H)[96:], w0[wo:].reshape(NO, H)[96:]) and np.array_equal(b1[bo + 96:], b0[bo + 96:])
    e, _, _ = make_net(xq, sizes, seed=4)
    e.set_precision(_capi.PRECISION_BF16)
    e.set_params(w1, b1)
    env = xq.VecEnv(n, seed=9)
    for _ in range(15):
        env.selfplay_step(None)
    qa, qb = d.q_boards(env, 96).cpu().numpy(), e.q_boards(env, 96).cpu().numpy()
    assert np.array_equal(qa.view(np.uint32), qb.view(np.uint32))
    e.set_params(w0, b1)
    assert not np.array_equal(qa, e.q_boards(env, 96).cpu().numpy())
    env.close(); d.close(); e.close()


def test_one_rank_communicator_has_the_same_bits(xq):
    """Clipping behind the all-reduce of a one-rank RCCL communicator: bit-identical to the same loop without one, 3 steps."""
    from cn_chess_ai_amd import dist as xd
    mk = lambda: xq.TrainerConfig(n_games=512, layer_sizes=(1260, 64, 64, 8100), replay_capacity=4096, minibatch=1024, td_net=0,
                                  target_sync_interval=3, seed=99, overlap_collect=1)
    ta, tb = xq.Trainer(mk()), xq.Trainer(mk())
    comm = xd.Comm(rank=0, world=1)
    tb.set_comm(comm)
    for t in (ta, tb):
        t.dqn.set_grad_clip(1e-3)
        for _ in range(3):
            t.learn_grads(); t.collect(); t.learn_apply(1)
    assert comm.info()["collectives"] == 3
    sa, sb = ta.dqn.grad_clip_stats(), tb.dqn.grad_clip_stats()
    assert sa == sb and sa["applies"] == 3 and sa["clipped"] >= 1
    assert same(ta.dqn.get_params(), tb.dqn.get_params())
    ta.close(); tb.close(); comm.close()


def test_doubled_gradient_with_world_size_two(xq):
    """"Sum over two identical ranks": the gradient buffer doubled in place, learn_apply(world_size=2).  Doubling is exact in S, in the
    square root and in both scales, so the coefficient and the parameters have the bits of the single-rank mean."""
    import torch
    from cn_chess_ai_amd import dist as xd
    sizes = (1260, 128, 8100)
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    cfg = xq.TrainerConfig(n_games=256, layer_sizes=sizes, replay_capacity=0, minibatch=256, td_net=0)
    outs = []
    for world in (2, 1):
        t = xq.Trainer(cfg, stream=C.c_void_p(s.cuda_stream))
        t.dqn.set_grad_clip(1e-3)
        ptr, n = t.dqn.grad_buffer()
        g = xd.wrap_device_floats(ptr, n)
        w0, _ = t.dqn.get_params()
        t.collect(); t.learn_grads()
        torch.cuda.synchronize()
        if world == 2:
            g.mul_(2.0)
            torch.cuda.synchronize()
        t.learn_apply(world_size=world)
        outs.append((t.dqn.grad_clip_stats(), w0) + t.dqn.get_params())
        t.close()
    torch.cuda.set_stream(torch.cuda.default_stream())
    (s2, w0, w2, b2), (s1, w0_, w1, b1) = outs
    assert s2 == s1 and s1["last_coef"] < 1.0 and s1["last_norm"] > 0
    assert np.array_equal(w0, w0_) and np.array_equal(w1, w2) and np.array_equal(b1, b2) and not np.array_equal(w1, w0)


def test_trainer_with_overlapped_collect_counts_every_apply(xq):
    cfg = xq.TrainerConfig(n_games=1024, layer_sizes=CFG2_NET, replay_capacity=8192, minibatch=1024, td_net=0, target_sync_interval=3,
                           seed=5, overlap_collect=1)
    t = xq.Trainer(cfg)
    t.dqn.set_grad_clip(1e-3)
    t.step(5)
    st = t.dqn.grad_clip_stats()
    assert st["applies"] == 5 and st["last_norm"] > 0 and 0 < st["last_coef"] <= 1.0
    t.close()


def test_backpropagate_is_never_clipped(xq):
    from cn_chess_ai_amd import _capi
    p, _, _ = make_net(xq, REF_NET, seed=2)
    q, _, _ = make_net(xq, REF_NET, seed=2)
    q.set_grad_clip(1e-9)
    x = br.one_hot(batch(xq, 1024, 61)[0][:4])
    tgt = np.zeros((4, 8100))
    p.backpropagate(x, tgt, 0.01, 1.0, _capi.BACKPROP_TEXTBOOK); q.backpropagate(x, tgt, 0.01, 1.0, _capi.BACKPROP_TEXTBOOK)
    assert same(p.get_params(), q.get_params())
    assert q.grad_clip_stats()["applies"] == 0
    p.close(); q.close()


def test_api_errors_and_what_the_setting_survives(xq):
    from cn_chess_ai_amd import _capi
    n = 1024
    S = batch(xq, n, 61)
    d, w, b = make_net(xq, REF_NET, seed=2)
    assert d.grad_clip() == 0.0
    with pytest.raises(xq.XqError) as e:
        d.grad_clip_stats()
    assert e.value.code == 2 and "off" in str(e.value)
    for bad in (-1.0, float("nan"), -math.inf):
        with pytest.raises(xq.XqError) as e:
            _capi.call("xq_dqn_set_grad_clip", d.handle, bad)
        assert e.value.code == 1
        with pytest.raises(ValueError):
            d.set_grad_clip(bad)
    assert d.grad_clip() == 0.0
    d.set_grad_clip(0.75)
    d.set_optimizer("adam"); d.set_optimizer("sgd"); d.set_params(w, b); d.updateTargetNetwork()
    assert d.grad_clip() == 0.75 and d.grad_clip_stats()["applies"] == 0
    _capi.call("xq_dqn_grad_clip_stats", d.handle, None, None, None, None)                   # any pointer may be NULL
    # refused while a TD step waits for its apply (as set_fused_apply)
    d.set_fused_apply(True)
    n = 8192
    rp = ring(xq, batch(xq, n, 77))
    rp.sample(n)
    d.td_grads_replay(rp, n, td_net=0, mode=0)
    with pytest.raises(xq.XqError) as e:
        d.set_grad_clip(0.0)
    assert e.value.code == 2 and "waiting" in str(e.value)
    d.apply_grads(1e-3, 1.0 / n)
    assert d.grad_clip_stats()["applies"] == 1
    # switching off and on again starts the counters afresh
    d.set_grad_clip(0.0); d.set_grad_clip(math.inf)
    assert d.grad_clip() == math.inf and d.grad_clip_stats() == dict(last_norm=0.0, last_coef=0.0, applies=0, clipped=0)
    rp.close(); d.close()


# ---- 6. reproducible --------------------------------------------------------------------------------------------------------------
def test_two_fresh_handles_give_the_same_bits(xq):
    n = 1024
    outs = []
    for _ in range(2):
        d, _, _ = make_net(xq, CFG2_NET, seed=8)
        d.set_grad_clip(1e-3)
        seq = []
        for i in range(3):
            S, A, R, D, S2 = batch(xq, n, 500 + i)
            d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=0.1, grad_scale=1.0 / n)
            seq.append(d.grad_clip_stats())
        outs.append((seq, d.get_params()))
        d.close()
    assert outs[0][0] == outs[1][0] and same(outs[0][1], outs[1][1])
    assert outs[0][0][-1]["clipped"] >= 1


# ---- the C++ facade ---------------------------------------------------------------------------------------------------------------
def test_facade_carries_the_clip_onto_the_trainers_network(xq):
    """xq::ChessAI::setGradClip forwards to its network (xq::DQN::gradClip reads it back, setOptimizer leaves it, a negative max_norm
    is std::invalid_argument, the statistics throw while off), and the batched train() takes it over: under SGD no weight moves
    further than updates x lr x max_norm (|lr c grad_scale g_i| <= lr c norm <= lr max_norm per update), and the same run with +inf
    moves them further."""
    import json
    import subprocess
    from test_clip_ref_cpu import build_clip_facade_probe
    exe = build_clip_facade_probe()
    max_norm = 1e-3
    out = subprocess.run([exe, "256", "100", "7", repr(max_norm)], check=True, capture_output=True, text=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["before"], r["set"], r["after_optimizer"]) == (0.0, max_norm, max_norm)
    assert r["negative_refused"] == 1 and r["stats_refused_while_off"] == 1 and r["fresh_applies"] == 0
    assert r["clip_updates"] > 0 and r["inf_updates"] > 0          # (other weights play other games: the two counts need not agree)
    assert 0 < r["clip_max_dw"] <= r["clip_updates"] * 0.001 * max_norm * (1 + 1e-5)
    assert r["inf_max_dw"] > r["clip_max_dw"]
