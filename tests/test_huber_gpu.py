"""The Huber TD loss (xq_dqn_set_td_loss: td_delta_kernel's Huber twin, qmax_refine2_kernel<256, true, HuberLoss>) and the TD-error
summary (xq_dqn_td_error_stats, td_error_stats_kernel) on the device — `pytest -m gpu`.

Reference: tests/huber_ref.py on tests/batch_ref.py (the Huber step is the squared step with per-sample weights clamp(e) / e), whose
error budget carries over unchanged.  kappa is always taken from the reference: the median of |e| over the live samples of the fp64
forward, so the reference alone puts half the samples on either side of the clamp.

The issue's "127 x 129 misaligned net" cannot take a TD step (the output-gradient kernel wants a last hidden width that is a multiple
of 4, tests/test_clip_gpu.py); the general path's misaligned case is that test's 1260-127-129-132-8100 under the textbook rule.

Largest err / bound observed on an MI355X: see profiles/NOTES.md ("Huber TD loss").
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import xqoracle as xo
import adam_ref as ar
import batch_ref as br
import huber_ref as hr
from test_adam_gpu import ring
from test_clip_gpu import SCALAR_TD_NET
from test_dqn_gpu import CFG2_NET, REF_NET, make_net, transitions, valid_indices
from test_td_full_size_gpu import PER, selfplay_batch

pytestmark = pytest.mark.gpu

F32_512_NET = [1260, 512, 8100]
CFG4_NET = [1260, 512, 512, 512, 8100]

# name: (net, n, TD rule, backprop mode, precision, screened + td-tail (the refine-fused delta), prioritized replay)
CASES = {
    "refine_fused_1024": (CFG2_NET, 1024, 0, 0, 0, True, False),
    "refine_fused_1000": (CFG2_NET, 1000, 0, 0, 0, True, False),       # a partly filled 32-sample block and a wave past the end
    "f32_256_fast": (CFG2_NET, 37, 0, 0, 0, False, False),
    "f32_512": (F32_512_NET, 37, 0, 0, 0, False, False),
    "general_128": (REF_NET, 37, 0, 0, 0, False, False),
    "general_127x129x132": (SCALAR_TD_NET, 37, 0, 1, 0, False, False),
    # (the bf16 cases: tests/test_config5_gpu.py's setup — transitions of the reference trace, rewards / 1000, its net seeds)
    "bf16_512": (CFG4_NET, 37, 0, 0, 1, False, False),
    "bf16_512_double": (CFG4_NET, 37, 2, 0, 1, False, False),
    "f32_256_fast_per": (CFG2_NET, 1024, 0, 0, 0, False, True),
    # (prioritized replay on the other three bodies of td_delta_kernel: importance weight in the delta, priority written back)
    "f32_512_per": (F32_512_NET, 37, 0, 0, 0, False, True),
    "general_128_per": (REF_NET, 37, 0, 0, 0, False, True),
    "bf16_512_per": (CFG4_NET, 37, 0, 0, 1, False, True),
}
BOTH_MODES = [(name, mode) for name in list(CASES)[:2] for mode in (0, 1)] + [(name, CASES[name][3]) for name in list(CASES)[2:]]


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


_SETUPS = {}


def setup(xq, name):
    """Batch, starting parameters, importance-weight priorities and the fp64 forward of a case, computed once and shared (never modified):
    (S, A, R, D, S2), (w0, b0, wt, bt), f, kappa"""
    if name in _SETUPS:
        return _SETUPS[name]
    sizes, n, rule, _, prec, _, per = CASES[name]
    wt = bt = None
    if prec:
        trace = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_trace.npz"))
        S, A, R, D, S2 = transitions(trace, valid_indices(trace, n, seed=4))
        R = (R / 1000.0).astype(np.float32)
        d, _, _ = make_net(xq, sizes, seed=9)
        if rule != 0:
            wt, bt = xo.init_weights(sizes, 78)
    else:
        S, A, R, D, S2 = selfplay_batch(xq, n, seed=300 + n + len(sizes), plies=20 + n % 21, every=7)
        d, _, _ = make_net(xq, sizes, seed=21)
        if rule != 0:
            wt, _ = xo.init_weights(sizes, 99)
            bt = np.random.default_rng(98).uniform(-0.05, 0.05, size=xo.nn_counts(sizes)[1])
    if rule != 0:
        d.set_params(wt, bt, net=1)
    d.set_precision(prec)
    w0, b0 = d.get_params()
    if rule != 0:
        wt, bt = d.get_params(1)
    d.close()
    slots = weights = prio = None
    if per:      # the draw depends on the ring's seed and priorities alone: done once here, repeated identically by every run
        rp = per_ring(xq, n, (S, A, R, D, S2))
        slots, weights = rp.sample_prioritized(n)
        rp.close()
        fS, fA, fR, fD, fS2 = S[slots], A[slots], R[slots], D[slots], S2[slots]
    else:
        fS, fA, fR, fD, fS2 = S, A, R, D, S2
    net = br.Net(sizes, w0, b0, prec)
    tnet = br.Net(sizes, wt, bt, prec) if rule != 0 else None
    f = br.forward(net, fS, fS2, fA, fR, fD, 0.99, rule, prec, target=tnet)
    e = np.abs(f.q - f.y)[f.live]
    kappa = float(np.median(e))
    # the reference alone puts half the samples on either side; at least a quarter must lie on each
    assert (e > kappa).sum() >= len(e) // 4 and (e <= kappa).sum() >= len(e) // 4, (name, kappa)
    _SETUPS[name] = ((S, A, R, D, S2), (w0, b0, wt, bt), f, kappa, net, slots, weights)
    return _SETUPS[name]


def per_prio(n):
    return np.random.default_rng(7).uniform(0.05, 2.0, size=n).astype(np.float32)


def per_ring(xq, n, batch):
    S, A, R, D, S2 = batch
    rp = xq.ReplayBuffer(n + n // 2, seed=0xFEED + n)
    rp.enable_per(*PER)
    rp.push(S, A, R, D, S2)
    rp.set_priorities(per_prio(n))
    rp.per_rebuild()
    return rp


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def grad_buffer(d):
    import torch
    from cn_chess_ai_amd import dist as xd
    ptr, k = d.grad_buffer()
    torch.cuda.synchronize()
    return xd.wrap_device_floats(ptr, k).cpu().numpy().copy()


def step_size(n):
    """(learning rate, gradient scale) of a case.  From 1000 samples up: tests/test_td_full_size_gpu.py's lr 1, scale 16 / n, the step
    batch_ref.TOLERANCES was set at (lr x scale between 0.001 and 0.016 there).  The 37-sample cases: tests/test_config5_gpu.py's lr 0.05
    with the mean gradient 1 / n, lr x scale = 0.00135 — scale 16 / n would make the step of a 37-sample batch 0.43, two hundred times
    what the bound was set at, where the device's absolute fp32 activation error (a few 2^-24 after layer 0's ~32 products), for which
    the bound has no term of its own, is no longer below the ulp of the stored weight that the bound grants."""
    return (1.0, 16.0 / n) if n >= 1000 else (0.05, 1.0 / n)


def run(xq, name, loss, mode=None, opt=None, want_stats=False):
    """One TD step of a case on a fresh handle.  loss: None (never asked), "squared", or kappa for huber.  opt: None (SGD) or "adam"
    (Adam + clip + tau = 0.01).  Returns a dict of everything the step leaves."""
    from cn_chess_ai_amd import _capi
    sizes, n, rule, mode0, prec, screened, per = CASES[name]
    mode = mode0 if mode is None else mode
    batch, (w0, b0, wt, bt), f, kappa, net, slots, weights = setup(xq, name)
    S, A, R, D, S2 = batch
    d = xq.DQN(sizes, 0.001, 0.99, seed=21)
    d.set_params(w0, b0)
    d.updateTargetNetwork()
    if rule != 0:
        d.set_params(wt, bt, net=1)
    d.set_precision(prec)
    d.set_qmax_mode(_capi.QMAX_SCREENED if screened else _capi.QMAX_FULL)
    d.set_td_tail(screened)
    if opt == "adam":
        d.set_optimizer("adam"); d.set_grad_clip(1e-3); d.set_target_tau(0.01)
    if loss == "squared":
        d.set_td_loss("squared")
    elif loss is not None:
        d.set_td_loss("huber", loss)
    lr, scale = step_size(n)
    out = dict(prio=None)
    d.kernel_stats(2)
    if per:
        rp = per_ring(xq, n, batch)
        got_slots, got_w = rp.sample_prioritized(n)
        assert np.array_equal(got_slots, slots) and np.array_equal(got_w, weights)
        d.td_grads_replay(rp, n, td_net=rule, mode=mode)
        d.apply_grads(lr, scale)
        out["q"], out["y"] = d.last_td_values(n)
        out["prio"] = rp.get_priorities(0, n + n // 2)
        rp.close()
    else:
        out["q"], out["y"] = d.td_update(S, S2, A, R, D, td_net=rule, mode=mode, learning_rate=lr, grad_scale=scale)
    out["launches"] = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
    out["loss"] = d.last_loss()
    out["params"] = d.get_params() + d.get_params(1) + (tuple(d.optimizer_state()[:2]) if opt == "adam" else ())
    out["grads"] = grad_buffer(d)
    out["lr"], out["scale"] = lr, scale
    if want_stats:
        out["stats"] = [d.td_error_stats(), d.td_error_stats()]
    d.close()
    return out


def same_step(a, b):
    return (all(np.array_equal(bits(x), bits(y)) for x, y in zip(a["params"], b["params"])) and len(a["params"]) == len(b["params"])
            and np.array_equal(bits(a["grads"]), bits(b["grads"])) and a["loss"] == b["loss"]
            and np.array_equal(bits(a["q"]), bits(b["q"])) and np.array_equal(bits(a["y"]), bits(b["y"]))
            and (a["prio"] is None) == (b["prio"] is None) and (a["prio"] is None or np.array_equal(bits(a["prio"]), bits(b["prio"]))))


# ---- 1. every delta path against fp64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", BOTH_MODES, ids=[f"{n}-mode{m}" for n, m in BOTH_MODES])
def test_huber_step_matches_the_fp64_reference_on_every_delta_path(xq, name, mode):
    """One TD step with huber(kappa): Q and y by batch_ref.check_q_y, every parameter by batch_ref.check_update with huber_ref's weights,
    last_loss against huber_ref.loss of the device's own (q, y) to 1e-6 relative; prioritized replay: the priorities written back are
    batch_ref.priorities of the RAW error.  The launch names tell that the intended kernel formed the delta.

    The learning rate and gradient scale of a case: step_size."""
    sizes, n, rule, _, prec, screened, per = CASES[name]
    _, _, f, kappa, net, slots, weights = setup(xq, name)
    r = run(xq, name, kappa, mode=mode)
    assert ("td_target_delta" not in r["launches"]) == screened, r["launches"]      # the refine blocks carried the delta, or the kernel did
    flipped, y_use = br.check_q_y(f, r["q"], r["y"], prec)
    hw = hr.weights(f, kappa, weights, y=y_use)
    u = br.accumulate(net, f, br.backward(net, f, mode, prec, hw, y=y_use), prec)
    w1, b1 = r["params"][:2]
    ratios = br.check_update(net, u, f, w1, b1, r["lr"], r["scale"], prec)
    loss_ref = hr.loss(f, float(np.float32(kappa)), y=r["y"].astype(np.float64), q=r["q"].astype(np.float64))
    print("huber", name, "mode", mode, "kappa", kappa, "flipped", len(flipped), "err/bound", {k: round(v, 4) for k, v in ratios.items()},
          "loss rel", abs(r["loss"] - loss_ref) / loss_ref)
    assert abs(r["loss"] - loss_ref) <= 1e-6 * loss_ref, (r["loss"], loss_ref)
    assert np.abs(w1 - net.w).max() > 0
    if per:
        # every sampled slot holds batch_ref.priorities of the RAW error — of the device's own Q and y to fp32 rounding (as
        # tests/test_td_full_size_gpu.py), and those are the reference's within check_q_y's bounds; every other slot keeps its priority
        fd = hr.copy_with(f, r["q"].astype(np.float64), r["y"].astype(np.float64))
        p_dev = br.priorities(fd, PER[2], PER[0])
        assert np.allclose(r["prio"][slots], p_dev, rtol=2e-5, atol=0), float(np.abs(r["prio"][slots] / p_dev - 1).max())
        assert np.abs(br.priorities(f, PER[2], PER[0], y=y_use) ** (1 / PER[0]) - p_dev ** (1 / PER[0])).max() < 2 * br.QTOL
        assert (np.abs(fd.q - fd.y) > 2 * kappa).any()          # ... raw: errors far above kappa are among them
        rest = np.setdiff1d(np.arange(n), slots)
        assert np.array_equal(r["prio"][rest], per_prio(n)[rest]) and not r["prio"][n:].any()


def test_the_reference_tells_huber_from_squared(xq):
    """The check above has teeth: the squared step's parameters fail it (same data, same bound)."""
    name = "general_128"
    sizes, n, rule, mode, prec, _, _ = CASES[name]
    _, _, f, kappa, net, _, _ = setup(xq, name)
    r = run(xq, name, None)
    _, y_use = br.check_q_y(f, r["q"], r["y"], prec)
    u = br.accumulate(net, f, br.backward(net, f, mode, prec, hr.weights(f, kappa, None, y=y_use), y=y_use), prec)
    ratios = br.update_ratios(net, u, r["params"][0], r["params"][1], r["lr"], r["scale"], prec)
    assert max(ratios.values()) > 10.0, ratios


# ---- 2. where the clamp sits, in fp32 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["refine_fused_1000", "f32_256_fast_per", "general_128", "f32_512"])
def test_output_bias_gradient_is_the_sum_of_the_clamped_deltas(xq, name):
    """delta restated in numpy float32 from the device's q, y (and the importance weights): delta = clamp(e) (1 - q q) isw.  gb_out[j] of
    the gradient buffer is the sum of the deltas of the samples with action j.  Bound per action: count_j 2^-23 sum |delta| — (count - 1)
    2^-24 sum|delta| for the fp32 summation in any order, 2^-23 |delta| per term for the roundings of delta itself; with importance weights one more 2^-23 per term (the device divides the raw weight by the raw maximum, the host list is
    already normalised).  A clamp behind (1 - q q) or behind isw moves the linear samples' deltas by q^2 or by 1 - isw relative."""
    sizes, n, rule, mode, prec, _, per = CASES[name]
    _, _, f, kappa, net, slots, weights = setup(xq, name)
    r = run(xq, name, kappa)
    q, y = r["q"].astype(np.float32), r["y"].astype(np.float32)
    k32 = np.float32(kappa)
    e = q - y
    c = np.minimum(np.maximum(e, -k32), k32)
    isw = np.ones(n, np.float32) if weights is None else weights.astype(np.float32)
    delta = (c * (np.float32(1.0) - q * q) * isw).astype(np.float64) * f.live
    gb = r["grads"][ar.layout(sizes)["bout"]:][:96].astype(np.float64)
    worst, wrong_place = 0.0, 0.0
    late = np.minimum(np.maximum((e * (np.float32(1.0) - q * q)), -k32), k32).astype(np.float64) * isw * f.live      # clamp behind (1 - q^2)
    for j in range(96):
        sel = f.A == j
        cnt = int(sel.sum())
        if cnt == 0:
            assert gb[j] == 0.0
            continue
        bound = cnt * 2.0 ** -23 * np.abs(delta[sel]).sum() * (2.0 if per else 1.0)
        worst = max(worst, abs(gb[j] - delta[sel].sum()) / bound)
        wrong_place = max(wrong_place, abs(late[sel].sum() - delta[sel].sum()) / bound)
    print("gb_out err/bound", name, worst, "a clamp behind (1 - q^2) would give", wrong_place)
    assert worst <= 1.0
    assert wrong_place > 1.0


# ---- 3. fixed point ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [None, "adam"], ids=["sgd", "adam_clip_tau"])
@pytest.mark.parametrize("name", list(CASES))
def test_huber_above_every_error_and_squared_have_the_bits_of_never_asked(xq, name, opt):
    """huber(inf) and huber(1e30): parameters (both nets; Adam's m and v), gradient buffer, loss, Q, y and priorities bit for bit those of
    the squared loss.  set_td_loss("squared") on a fresh handle: those bits and the launch names and counts of a handle never asked.

    This holds because every loss forms 1 - q^2 with the same two roundings (td_dtanh): an fma there moves a delta by an ulp about once
    in a thousand samples, which only the large batches show."""
    never = run(xq, name, None, opt=opt)
    asked = run(xq, name, "squared", opt=opt)
    assert same_step(never, asked) and asked["launches"] == never["launches"]
    for kappa in (math.inf, 1e30):
        h = run(xq, name, kappa, opt=opt)
        assert same_step(never, h), (name, kappa)
        assert h["launches"] == never["launches"]                                    # same brackets: the twin kernel rides in the same ones
    assert np.abs(never["params"][0] - setup(xq, name)[1][0]).max() > 0


# ---- 4. statistics ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["refine_fused_1000", "general_128", "bf16_512_double", "f32_256_fast_per"])
def test_td_error_stats_against_the_reference(xq, name):
    sizes, n, rule, mode, prec, _, per = CASES[name]
    _, _, f, kappa, net, _, _ = setup(xq, name)
    for loss in (kappa, None):
        r = run(xq, name, loss, want_stats=True)
        st, again = r["stats"]
        assert st == again                                                            # two calls give the same record
        k = kappa if loss is not None else math.inf
        ref = hr.stats(r["q"], r["y"], f.live, k)
        assert st["live"] == ref["live"] == int(f.live.sum()) and st["max_abs"] == ref["max_abs"] and st["linear"] == ref["linear"]
        tol = n * 2.0 ** -52
        assert abs(st["mean_abs"] - ref["mean_abs"]) <= tol * ref["mean_abs"]
        assert abs(st["mean_loss"] - ref["mean_loss"]) <= tol * ref["mean_loss"]
        # last_loss is the fp32 per-sample loss summed on the host: the same quantity to fp32 rounding
        assert abs(st["mean_loss"] * st["live"] - r["loss"]) <= 1e-6 * r["loss"]
        if loss is None:
            assert st["linear"] == 0
        else:
            # against the fp64 forward's own e: 1e-4 is the project's Q tolerance (fp32 nets; the bf16 net's is BF16_QTOL, and where a
            # Double DQN arg-max flipped the reference takes the device's y, as check_q_y grants)
            qtol = br.BF16_QTOL if prec else 1e-4
            _, y_use = br.check_q_y(f, r["q"], r["y"], prec)
            e64 = np.abs(f.q - (y_use if rule == 2 else f.y))[f.live]
            lo, hi = int((e64 > kappa + qtol).sum()), int((e64 > kappa - qtol).sum())
            print("linear", name, lo, st["linear"], hi)
            assert lo <= st["linear"] <= hi, (lo, st["linear"], hi)
            assert 0 < st["linear"] < st["live"]


def test_stats_count_only_live_samples(xq):
    """Empty slots (action -1) are no samples: live, the means and the maximum leave them out."""
    name = "general_128"
    sizes, n = CASES[name][0], CASES[name][1]
    (S, A, R, D, S2), (w0, b0, _, _), f, kappa, net, _, _ = setup(xq, name)
    A2 = A.copy(); A2[::5] = -1
    d = xq.DQN(sizes, 0.001, 0.99, seed=21)
    d.set_params(w0, b0)
    d.set_td_loss("huber", kappa)
    q, y = d.td_update(S, S2, A2, R, D, td_net=0, mode=0, learning_rate=0.0, grad_scale=1.0)
    st = d.td_error_stats()
    ref = hr.stats(q, y, A2 >= 0, kappa)
    assert st["live"] == int((A2 >= 0).sum()) == ref["live"] < n
    assert st["max_abs"] == ref["max_abs"] and st["linear"] == ref["linear"]
    assert abs(st["mean_abs"] - ref["mean_abs"]) <= n * 2.0 ** -52 * ref["mean_abs"]
    d.close()


# ---- 5. composition ---------------------------------------------------------------------------------------------------------------
def test_one_rank_communicator_has_the_same_bits(xq):
    from cn_chess_ai_amd import dist as xd
    mk = lambda: xq.TrainerConfig(n_games=512, layer_sizes=(1260, 64, 64, 8100), replay_capacity=4096, minibatch=1024, td_net=0,
                                  target_sync_interval=3, seed=99, overlap_collect=1)
    ta, tb, tc = xq.Trainer(mk()), xq.Trainer(mk()), xq.Trainer(mk())
    comm = xd.Comm(rank=0, world=1)
    tb.set_comm(comm)
    for t, loss in ((ta, 0.05), (tb, 0.05), (tc, None)):
        if loss:
            t.dqn.set_td_loss("huber", loss)
        for _ in range(3):
            t.learn_grads(); t.collect(); t.learn_apply(1)
    assert comm.info()["collectives"] == 3
    assert ta.dqn.td_error_stats() == tb.dqn.td_error_stats() and ta.dqn.td_error_stats()["linear"] > 0
    pa, pb, pc = ta.dqn.get_params(), tb.dqn.get_params(), tc.dqn.get_params()
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert not np.array_equal(pa[0], pc[0])                                           # and Huber is not the squared loss here
    ta.close(); tb.close(); tc.close(); comm.close()


def test_overlapped_trainer_with_huber_equals_its_sequential_definition(xq):
    """tests/test_trainer_gpu.py's composition with Huber on, 8 steps: bit for bit."""
    import torch
    from ring_window_ref import overlap_window
    n, cap, minibatch, iters, sizes, kappa = 64, 256, 48, 8, CFG2_NET, 0.05
    seed, first = 99, 7
    cfg = xq.TrainerConfig(n_games=n, layer_sizes=sizes, learning_rate=0.01, gamma=0.99, epsilon=0.2, replay_capacity=cap,
                           minibatch=minibatch, td_net=1, backprop_mode=0, target_sync_interval=3, mean_gradient=1, seed=seed,
                           first_game_id=first, collects_per_update=1, overlap_collect=1)
    t = xq.Trainer(cfg)
    t.dqn.set_td_loss("huber", kappa)
    w0, b0 = t.dqn.get_params()
    t.step(iters)
    tw, tb = t.dqn.get_params()
    tboards, tmeta = t.env.get_state()
    tst = t.dqn.td_error_stats()
    env = xq.VecEnv(n, seed=seed, first_game_id=first)
    d = xq.DQN(sizes, 0.01, 0.99, seed=1)
    d.set_params(w0, b0); d.updateTargetNetwork()
    d.set_td_loss("huber", kappa)
    rp = xq.ReplayBuffer(cap, seed=seed + 0x1234567 + first)

    def collect():
        q = d.q_boards(env, 96)
        env.selfplay_step_dev(q.data_ptr(), 96, 0.2, replay=rp)
        torch.cuda.synchronize()

    for it in range(iters):
        size, _, total = rp.stats()
        start, count = overlap_window(size, total, cap, n)
        if count <= 0:
            collect()
            rp.sample(minibatch)
            d.td_grads_replay(rp, minibatch, td_net=1, mode=0)
        else:
            rp.sample_window(minibatch, start, count)
            d.td_grads_replay(rp, minibatch, td_net=1, mode=0)
            collect()
        d.apply_grads(0.01, 1.0 / minibatch)
        if (it + 1) % 3 == 0:
            d.updateTargetNetwork()
    w, b = d.get_params()
    boards, meta = env.get_state()
    assert np.array_equal(boards, tboards) and np.array_equal(meta, tmeta)
    assert np.array_equal(w, tw) and np.array_equal(b, tb) and np.abs(w - w0).max() > 0
    st = d.td_error_stats()
    assert st == tst and 0 < st["linear"] <= st["live"]
    t.close(); env.close(); d.close(); rp.close()


def test_backpropagate_is_never_affected(xq):
    from cn_chess_ai_amd import _capi
    p, _, _ = make_net(xq, REF_NET, seed=2)
    q, _, _ = make_net(xq, REF_NET, seed=2)
    q.set_td_loss("huber", 1e-6)
    x = br.one_hot(setup(xq, "general_128")[0][0][:4])
    tgt = np.zeros((4, 8100))
    p.backpropagate(x, tgt, 0.01, 1.0, _capi.BACKPROP_TEXTBOOK); q.backpropagate(x, tgt, 0.01, 1.0, _capi.BACKPROP_TEXTBOOK)
    assert all(np.array_equal(a, b) for a, b in zip(p.get_params(), q.get_params()))
    p.close(); q.close()


def test_api_errors_and_what_the_setting_survives(xq, tmp_path):
    from cn_chess_ai_amd import _capi
    d, w, b = make_net(xq, REF_NET, seed=2)
    assert d.td_loss() == dict(kind="squared", kappa=1.0)
    with pytest.raises(xq.XqError) as e:
        d.td_error_stats()
    assert e.value.code == 2 and "no TD step" in str(e.value)
    for kind, bad in ((1, 0.0), (1, -1.0), (1, float("nan")), (1, -math.inf), (1, 1e-60), (2, 1.0), (-1, 1.0)):
        with pytest.raises(xq.XqError) as e:
            _capi.call("xq_dqn_set_td_loss", d.handle, kind, bad)
        assert e.value.code == 1
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            d.set_td_loss("huber", bad)
    with pytest.raises(ValueError):
        d.set_td_loss("absolute")
    assert d.td_loss() == dict(kind="squared", kappa=1.0)
    d.set_td_loss("squared", kappa=-5.0)                                              # kappa is ignored for the squared loss
    d.set_td_loss("huber", math.inf)
    assert d.td_loss() == dict(kind="huber", kappa=math.inf)
    d.set_td_loss("huber", 0.75)
    path = str(tmp_path / "m.bin")
    d.saveModel(path)
    d.set_optimizer("adam"); d.set_optimizer("sgd"); d.set_grad_clip(1.0); d.set_target_tau(0.5); d.set_params(w, b)
    d.loadModel(path); d.updateTargetNetwork(); d.set_precision(_capi.PRECISION_BF16); d.set_precision(_capi.PRECISION_F32)
    assert d.td_loss() == dict(kind="huber", kappa=0.75)
    d.set_td_loss("squared")
    assert d.td_loss() == dict(kind="squared", kappa=0.75)                            # the last kappa is kept
    d.set_td_loss("huber", 0.75)
    d.set_grad_clip(0.0); d.set_target_tau(0.0)
    # refused while a TD step waits for its apply (as set_fused_apply); the statistics may be read there
    d.set_fused_apply(True)
    n = 1024
    S = selfplay_batch(xq, n, seed=61, plies=13, every=7)
    rp = ring(xq, S)
    rp.sample(n)
    d.td_grads_replay(rp, n, td_net=0, mode=0)
    with pytest.raises(xq.XqError) as e:
        d.set_td_loss("squared")
    assert e.value.code == 2 and "waiting" in str(e.value)
    assert d.td_error_stats()["live"] == n
    d.apply_grads(1e-3, 1.0 / n)
    d.set_td_loss("squared")
    _capi.call("xq_dqn_td_error_stats", d.handle, None, None, None, None, None)        # any pointer may be NULL
    _capi.call("xq_dqn_get_td_loss", d.handle, None, None)
    rp.close(); d.close()


def test_facade_carries_the_loss_onto_the_trainers_network(xq):
    """xq::ChessAI::setTdLoss forwards to its network (xq::DQN::tdLoss reads it back; setOptimizer, setGradClip and setTargetTau leave it;
    kappa = 0 is std::invalid_argument; the statistics throw before the first TD step), and the batched train() takes it over: under SGD
    with the mean gradient no output-layer weight moves further than updates x lr x kappa (|delta| <= kappa, |a| <= 1, so every entry of
    the mean output-layer gradient is at most kappa), and the same run under the squared loss moves them further."""
    import json
    import subprocess
    from test_huber_ref_cpu import build_huber_facade_probe
    exe = build_huber_facade_probe()
    kappa = 1e-3
    out = subprocess.run([exe, "256", "100", "7", repr(kappa)], check=True, capture_output=True, text=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["before"], r["set_kind"], r["set_kappa"], r["after_kind"], r["after_kappa"]) == (0, 1, kappa, 1, kappa)
    assert r["zero_refused"] == 1 and r["stats_refused_before_step"] == 1
    assert r["huber_updates"] > 0 and r["squared_updates"] > 0
    assert 0 < r["huber_max_dw"] <= r["huber_updates"] * 0.001 * kappa * (1 + 1e-5)
    assert r["squared_max_dw"] > r["huber_max_dw"]
