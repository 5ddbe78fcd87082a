"""Full-size TD updates against the batched fp64 reference (tests/batch_ref.py) — `pytest -m gpu`.

The production batch sizes run code paths that small batches never reach: layer-0 gradient chunks of 1024 / 2048 samples, the bf16
planes of the delta product's epilogue (whole chunks only), the select head riding on the last hidden product (n >= 2048, n % 64 == 0),
128x128 tiles and the persistent walk at >= 512 tiles, split-K slab counts and grids that depend on n.  Each case below runs ONE TD
step on self-play transitions and checks every Q(s,a), every y, the loss and every parameter against the reference, with the
bound of batch_ref.TOLERANCES and the exact checks of batch_ref.check_update.
"""
import numpy as np
import pytest

import batch_ref as br
import xqoracle as xo
from test_dqn_gpu import CFG2_NET, REF_NET, make_net

pytestmark = pytest.mark.gpu

CFG4_NET = [1260, 512, 512, 512, 8100]
PER = (0.6, 0.4, 1e-3)          # alpha, beta, eps


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def selfplay_batch(xq, n, seed, plies, every, reward_div=100.0):
    """n transitions of random self-play after `plies` plies; every `every`-th sample terminal"""
    env = xq.VecEnv(n, seed=seed)
    for _ in range(plies):
        env.selfplay_step(None)
    S, _ = env.get_state()
    res = env.selfplay_step(None)
    S2, _ = env.get_state()
    env.close()
    A = (res["action"] % 90).astype(np.int32)
    R = (res["reward"] / reward_div).astype(np.float32)
    D = res["done"].copy()
    D[::every] = 1
    return S, A, R, D, S2


# name: (net, n, td_rule, mode, precision, switches, reward divisor, PER)
HEADLINE = dict(qmax="screened", derive=True, fused=True, tail=True, l0grad=1)
CASES = {
    "headline": (CFG2_NET, 8192, 0, 0, 0, HEADLINE, 100.0, False),
    "headline_l0grad_segmented": (CFG2_NET, 8192, 0, 0, 0, dict(HEADLINE, l0grad=0), 100.0, False),
    "headline_td_tail_off": (CFG2_NET, 8192, 0, 0, 0, dict(HEADLINE, tail=False), 100.0, False),
    "headline_qmax_full": (CFG2_NET, 8192, 0, 0, 0, dict(HEADLINE, qmax="full"), 100.0, False),
    "target_net_mode1": (CFG2_NET, 8192, 1, 1, 0, HEADLINE, 100.0, False),
    "ref_net_raw_rewards": (REF_NET, 4096, 0, 0, 0, HEADLINE, 1.0, False),
    "config4": (CFG4_NET, 8192, 0, 0, 0, HEADLINE, 100.0, False),
    "config5_bf16_full": (CFG4_NET, 16384, 2, 0, 2, HEADLINE, 100.0, True),
    "config5_bf16": (CFG4_NET, 16384, 2, 0, 1, HEADLINE, 100.0, True),
    "ragged_2047": (CFG2_NET, 2047, 0, 0, 0, HEADLINE, 100.0, False),
    "ragged_3000": (CFG2_NET, 3000, 0, 0, 0, HEADLINE, 100.0, False),
    "ragged_16383": (CFG2_NET, 16383, 0, 0, 0, HEADLINE, 100.0, False),
    "whole_16384": (CFG2_NET, 16384, 0, 0, 0, HEADLINE, 100.0, False),
}


def run_case(xq, name, seed=0):
    """One TD step of case `name` on the device and in the reference; checks Q, y, the loss (and the PER priorities) and returns
    what the parameter comparison needs: (net before the step, forward, update, new w, new b, lr, scale, precision)."""
    from cn_chess_ai_amd import _capi
    sizes, n, rule, mode, prec, sw, rdiv, per = CASES[name]
    S, A, R, D, S2 = selfplay_batch(xq, n, seed=1000 + n + seed, plies=20 + (n + seed) % 21, every=7 + seed % 5, reward_div=rdiv)
    d, _, _ = make_net(xq, sizes, seed=21 + seed)
    if rule != 0:                                             # a target net that differs from the online net
        wt, _ = xo.init_weights(sizes, 99 + seed)
        bt = np.random.default_rng(98 + seed).uniform(-0.05, 0.05, size=xo.nn_counts(sizes)[1])
        d.set_params(wt, bt, net=1)
    d.set_precision(prec)
    d.set_qmax_mode(_capi.QMAX_SCREENED if sw["qmax"] == "screened" else _capi.QMAX_FULL)
    d.set_l0_derive(sw["derive"])
    d.set_fused_apply(sw["fused"])
    d.set_td_tail(sw["tail"])
    d.set_l0_grad_mode(sw["l0grad"])
    w0, b0 = d.get_params()                                   # what the device starts from (fp32 values)
    wt0, bt0 = d.get_params(1)
    lr = 1.0 if rdiv > 1.0 else 0.01
    scale = 16.0 / n
    weights = None
    if per:
        cap = n + n // 2
        rp = xq.ReplayBuffer(cap, seed=0xFEED + n)
        rp.enable_per(*PER)
        rp.push(S, A, R, D, S2)
        prio = np.random.default_rng(7 + seed).uniform(0.05, 2.0, size=n).astype(np.float32)
        rp.set_priorities(prio)
        rp.per_rebuild()
        slots, weights = rp.sample_prioritized(n)
        d.td_grads_replay(rp, n, td_net=rule, mode=mode)
        d.apply_grads(lr, scale)
        q_dev, y_dev = d.last_td_values(n)
        S, A, R, D, S2 = S[slots], A[slots], R[slots], D[slots], S2[slots]
    else:
        q_dev, y_dev = d.td_update(S, S2, A, R, D, td_net=rule, mode=mode, learning_rate=lr, grad_scale=scale)
    loss_dev = d.last_loss()
    new_w, new_b = d.get_params()
    net = br.Net(sizes, w0, b0, prec)
    tnet = br.Net(sizes, wt0, bt0, prec) if rule != 0 else None
    f = br.forward(net, S, S2, A, R, D, 0.99, rule, prec, target=tnet)
    flipped, y_use = br.check_q_y(f, q_dev, y_dev, prec)
    loss_ref = br.loss(f, y_use)
    assert abs(loss_dev - loss_ref) <= br.LOSS_RTOL[prec] * loss_ref, (loss_dev, loss_ref)
    bk = br.backward(net, f, mode, prec, weights, y=y_use)
    u = br.accumulate(net, f, bk, prec)
    if per:
        p2 = rp.get_priorities(0, cap)
        # every sampled slot holds (|Q(s,a) - y| + eps)^alpha of the device's own Q and y (duplicates: of each of them), and those
        # are the reference's within check_q_y's bounds; every other slot keeps its priority
        p_dev = (np.abs(q_dev.astype(np.float64) - y_dev) + PER[2]) ** PER[0]
        assert np.allclose(p2[slots], p_dev, rtol=2e-5, atol=0), float(np.abs(p2[slots] / p_dev - 1).max())
        rest = np.setdiff1d(np.arange(n), slots)
        assert np.array_equal(p2[rest], prio[rest]) and not p2[n:].any()
        rp.close()
    d.close()
    return net, f, u, new_w, new_b, lr, scale, prec, flipped


@pytest.mark.parametrize("name", list(CASES))
def test_full_size_td_update_matches_the_batched_reference(xq, name):
    net, f, u, new_w, new_b, lr, scale, prec, flipped = run_case(xq, name)
    ratios = br.check_update(net, u, f, new_w, new_b, lr, scale, prec)
    print(name, "flipped", len(flipped), "err/bound", {k: round(v, 4) for k, v in ratios.items()})
