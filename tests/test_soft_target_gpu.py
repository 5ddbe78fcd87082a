"""Soft (Polyak) target update of xq_dqn_apply_grads (xq_dqn_set_target_tau: the SOFT forms of the four apply kernels, soft_target_kernel)
and xq_dqn_soft_update_target on the device — `pytest -m gpu`.

Reference and bounds: tests/polyak_ref.py (fp64 restatement, the derived one-step rounding bound, the K-step budget).

Two cases differ from the first draft of this suite, both because the library refuses or bypasses what the draft assumed:
  * 1260-127-129-8100 (MISALIGNED_NET) cannot take a TD step: the output-gradient kernel wants a last hidden width that is a multiple of
    4.  It serves wherever gradients are injected and for the explicit call; the trajectory of real TD steps through the scalar loops
    runs on 1260-127-129-132-8100 with the textbook backward rule, the net tests/test_clip_gpu.py uses for the same reason.
  * Exact screening engages from 897 samples on (64 x ceil(n / 128) >= 512 tiles); at n = 512 XQ_QMAX_SCREENED runs the full product and
    "screened == full, bit for bit" holds by construction.  That leg stays, and a leg at n = 1024, where qmax_stats() shows every step
    screened, is added: bit-exact against a screened twin whose target is re-set through set_params before every step (which makes the
    screen convert every row of its shadow afresh), and within the existing screened-against-full bar (2e-6, tests/test_dqn_gpu.py:
    the two differ in summation order with or without a soft update) of a twin on the full product.

Every test prints the largest err / bound it saw (`pytest -s`); profiles/NOTES.md ("Soft target update") is where they are recorded.
"""
import json
import subprocess

import numpy as np
import pytest

import adam_ref as ar
import clip_ref as cr
import polyak_ref as pr
from test_adam_gpu import MISALIGNED_NET, ring
from test_clip_gpu import SCALAR_TD_NET, batch, seeded_gradient
from test_dqn_gpu import CFG2_NET, REF_NET, make_net

pytestmark = pytest.mark.gpu
NETS = pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET, MISALIGNED_NET], ids=["256x256_vec4", "128_vec4", "127x129_scalar"])


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def flat(d, net=0):
    """all parameters of one net as fp32, weights then biases (reference layout)"""
    w, b = d.get_params(net)
    return np.concatenate([w, b]).astype(np.float32)


def seeded_params(sizes, seed):
    """fp32-representable parameters, non-zero everywhere"""
    rng = np.random.default_rng(seed)
    nw = sum(a * b for a, b in zip(sizes[:-1], sizes[1:]))
    nb = sum(sizes[1:])
    w = rng.uniform(0.001, 0.05, size=nw) * rng.choice([-1.0, 1.0], size=nw)
    b = rng.uniform(0.001, 0.05, size=nb) * rng.choice([-1.0, 1.0], size=nb)
    return w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)


def td_mask(sizes):
    cw, cb = ar.covered(sizes)
    return np.concatenate([cw, cb])


def inject(xq, handles, g):
    import torch
    from cn_chess_ai_amd import dist as xd
    for h in handles:
        ptr, n = h.grad_buffer()
        xd.wrap_device_floats(ptr, n).copy_(torch.from_numpy(g))
    torch.cuda.synchronize()


def launches(d):
    return {s["name"]: s["launches"] for s in d.kernel_stats(0)}


def check_step(t_old, p_new, t_new, tau, where=None):
    """largest err / bound of the device's target against polyak_ref over the elements `where` selects"""
    ref, bound = pr.one_step_bound(t_old, p_new, pr.tau32(tau))
    r = np.abs(t_new.astype(np.float64) - ref) / bound
    return float(r.max() if where is None else r[where].max())


# ---- 1. one step, gradient injected -------------------------------------------------------------------------------------------------
@NETS
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_one_step_with_injected_gradient(xq, sizes, opt):
    """Seeded gradients written straight into the gradient buffer, SGD and Adam, clipping off and on, tau 0.005 and 0.3, against a twin
    handle with tau = 0 that gets the same gradients.  (a) Target and online set to different values everywhere (set_params on both nets:
    the whole-buffer kernel follows the apply): online bits those of the twin, every target parameter inside and outside the TD segments
    within the one-step bound of polyak_ref.step(t_old, p_new_dev, tau32), the twin's target untouched.  (b) After update_target() (the
    SOFT form of the apply kernel, no second launch), two applies: the same checks on the TD segments, the rest of the target keeps the
    online net's bits.  1260-127-129: every segment but layer 0 takes the scalar loops, and the whole-buffer kernel its scalar tail."""
    d, e = xq.DQN(sizes, seed=1), xq.DQN(sizes, seed=1)
    n = d.grad_buffer()[1]
    cov = td_mask(sizes)
    rng = np.random.default_rng(sizes[1] + (7 if opt == "adam" else 0))
    lr, gs = 1e-3, 1.0 / 3.0
    wo, bo = seeded_params(sizes, 41)
    wt, bt = seeded_params(sizes, 42)
    worst = dict(whole_td=0.0, whole_rest=0.0, fused=0.0)
    for h in (d, e):
        h.set_optimizer(opt)
    for clip in (False, True):
        for tau in (0.005, 0.3):
            g = seeded_gradient(rng, n, "spread")
            for h in (d, e):
                h.set_params(wo, bo); h.set_params(wt, bt, net=1)
                h.set_grad_clip(0.25 * cr.norm(g, gs) if clip else 0.0)
            d.set_target_tau(tau)
            assert d.target_tau() == tau and e.target_tau() == 0.0
            t_old = flat(d, 1)
            inject(xq, (d, e), g)
            d.kernel_stats(2)
            d.apply_grads(lr, gs); e.apply_grads(lr, gs)
            st = launches(d)
            assert st.get("soft_target") == 1 and st["adam_apply" if opt == "adam" else "sgd_apply"] == 1
            p_new, t_new = flat(d), flat(d, 1)
            assert np.array_equal(bits(p_new), bits(flat(e)))
            assert np.array_equal(bits(flat(e, 1)), bits(t_old))
            assert not np.array_equal(p_new[cov], np.concatenate([wo, bo]).astype(np.float32)[cov])
            worst["whole_td"] = max(worst["whole_td"], check_step(t_old, p_new, t_new, tau, cov))
            worst["whole_rest"] = max(worst["whole_rest"], check_step(t_old, p_new, t_new, tau, ~cov))
            assert (t_new != t_old).mean() > 0.9
            # (b) the nets in step outside the TD segments: the update rides in the apply kernel
            d.updateTargetNetwork(); e.updateTargetNetwork()
            assert d.target_tau() == tau
            for k in range(2):
                g = seeded_gradient(rng, n, "spread")
                t_old = flat(d, 1)
                inject(xq, (d, e), g)
                d.kernel_stats(2)
                d.apply_grads(lr, gs); e.apply_grads(lr, gs)
                assert "soft_target" not in launches(d)
                p_new, t_new = flat(d), flat(d, 1)
                assert np.array_equal(bits(p_new), bits(flat(e)))
                worst["fused"] = max(worst["fused"], check_step(t_old, p_new, t_new, tau, cov))
                assert np.array_equal(bits(t_new[~cov]), bits(p_new[~cov])) and np.array_equal(bits(t_new[~cov]), bits(t_old[~cov]))
                moved = (t_new != t_old) & cov
                assert moved.sum() > 0.2 * cov.sum()
                assert not np.array_equal(t_new[cov], p_new[cov])
    print("soft target one-step err/bound", sizes, opt, {k: round(v, 4) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
    d.close(); e.close()


@pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET], ids=["256x256", "128"])
@pytest.mark.parametrize("form", ["whole", "fused"])
def test_bf16_shadow_of_the_target_is_the_rounded_new_value(xq, sizes, form):
    """XQ_PRECISION_BF16, two soft applies (whole-buffer form: the nets differ everywhere; fused form: after update_target()).  A second
    handle that gets the new target through set_params(target) — which converts every weight afresh — gives the same Q bits from the
    target net on every board and all 8100 outputs, so the shadow the kernels wrote is bf16(t'); with the old target it does not."""
    from cn_chess_ai_amd import _capi
    d = xq.DQN(sizes, seed=1)
    d.set_precision(_capi.PRECISION_BF16)
    wo, bo = seeded_params(sizes, 41)
    wt, bt = seeded_params(sizes, 42)
    d.set_params(wo, bo); d.set_params(wt, bt, net=1)
    if form == "fused":
        d.updateTargetNetwork()
    d.set_target_tau(0.3)
    n = d.grad_buffer()[1]
    rng = np.random.default_rng(5)
    t_first = d.get_params(1)
    for _ in range(2):
        inject(xq, (d,), seeded_gradient(rng, n, "spread"))
        d.kernel_stats(2)
        d.apply_grads(1e-3, 1.0 / 3.0)
        assert ("soft_target" in launches(d)) == (form == "whole")
    t_w, t_b = d.get_params(1)
    assert not np.array_equal(t_w, t_first[0])
    env = xq.VecEnv(256, seed=9)
    for _ in range(15):
        env.selfplay_step(None)
    e = xq.DQN(sizes, seed=2)
    e.set_precision(_capi.PRECISION_BF16)
    e.set_params(t_w, t_b, net=1)
    qa, qb = d.q_boards(env, 8100, net=1).cpu().numpy(), e.q_boards(env, 8100, net=1).cpu().numpy()
    assert np.array_equal(qa.view(np.uint32), qb.view(np.uint32))
    e.set_params(*t_first, net=1)
    assert not np.array_equal(qa, e.q_boards(env, 8100, net=1).cpu().numpy())
    env.close(); d.close(); e.close()


# ---- 2. fixed point: touched-only == whole-buffer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [CFG2_NET, REF_NET], ids=["256x256", "128"])
def test_touched_only_form_has_the_bits_of_the_whole_buffer_form(xq, sizes):
    """Two handles with identical parameters.  A: update_target(), so the apply kernel walks the TD segments only.  B: the same, then
    set_params(target) with the very same values, so the whole-buffer kernel follows every apply.  Six real TD steps on 512 self-play
    transitions with tau = 0.01: after every step the two target nets are bit-equal, and rows >= 96 of the target's W_out and their biases
    have the online net's bits."""
    n, tau = 512, 0.01
    A, w, b = make_net(xq, sizes, seed=5)
    B, _, _ = make_net(xq, sizes, seed=5)
    B.set_params(*B.get_params(1), net=1)
    cov = td_mask(sizes)
    t0 = flat(A, 1)
    for h in (A, B):
        h.set_target_tau(tau)
        h.kernel_stats(2)
    for i in range(6):
        S, Ac, R, D, S2 = batch(xq, n, 61 + (i & 1))
        for h in (A, B):
            h.td_update(S, S2, Ac, R, D, td_net=0, mode=0, learning_rate=0.5, grad_scale=1.0 / n)
        tA, tB, pA = flat(A, 1), flat(B, 1), flat(A)
        assert np.array_equal(bits(tA), bits(tB)), i
        assert np.array_equal(bits(pA), bits(flat(B)))
        assert np.array_equal(bits(tA[~cov]), bits(pA[~cov])) and (~cov).sum() == (sizes[-1] - 96) * (sizes[-2] + 1)
    assert (tA[cov] != t0[cov]).sum() > 1000 and (tA[cov] != pA[cov]).sum() > 1000
    sa, sb = launches(A), launches(B)
    assert "soft_target" not in sa and sb["soft_target"] == 6 and sa["sgd_apply"] == sb["sgd_apply"] == 6
    A.close(); B.close()


# ---- 3. trajectory ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,n,mode", [(SCALAR_TD_NET, 300, 1), (CFG2_NET, 512, 0)], ids=["127x129x132_scalar", "256x256"])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_target_follows_the_fp64_recursion_over_twenty_td_steps(xq, sizes, n, mode, opt):
    """20 TD steps with tau = 0.01; the online net is read back after each.  The target stays within the K-step budget (sum of the
    one-step bounds) of the fp64 recursion t <- t + tau32 (p_k - t) over those snapshots, on every parameter."""
    tau = 0.01
    d, _, _ = make_net(xq, sizes, seed=5)
    d.set_optimizer(opt)
    d.set_target_tau(tau)
    t = flat(d, 1)
    t0 = t.copy()
    B = pr.Budget(t)
    worst = 0.0
    for k in range(20):
        S, A, R, D, S2 = batch(xq, n, 61 + k % 3)
        d.td_update(S, S2, A, R, D, td_net=0, mode=mode, learning_rate=0.2 if opt == "sgd" else 1e-3, grad_scale=1.0 / n)
        p, t1 = flat(d), flat(d, 1)
        ref, bound = B.advance(t, p, pr.tau32(tau))
        worst = max(worst, float((np.abs(t1.astype(np.float64) - ref) / bound).max()))
        t = t1
    print("soft target trajectory err/budget", sizes, opt, round(worst, 4))
    assert worst <= 1.0
    cov = td_mask(sizes)
    assert (t[cov] != t0[cov]).mean() > 0.05 and np.array_equal(bits(t[~cov]), bits(t0[~cov]))
    # the recursion is not the identity and not the copy: it sits between the two
    assert np.abs(t.astype(np.float64) - t0)[cov].max() > 100 * bound[cov].max()
    assert np.abs(t.astype(np.float64) - p)[cov].max() > 100 * bound[cov].max()
    d.close()


# ---- 4. bounds of tau ---------------------------------------------------------------------------------------------------------------
def test_tau_one_is_the_hard_copy_shadow_included(xq):
    """tau = 1 through the setting and through soft_update_target equals update_target() bit for bit; under bf16 the target's shadow too
    (the target net's Q bits on every board and all 8100 outputs are those of the handle that copied)."""
    from cn_chess_ai_amd import _capi
    sizes = REF_NET
    wo, bo = seeded_params(sizes, 41)
    wt, bt = seeded_params(sizes, 42)
    hs = [xq.DQN(sizes, seed=1) for _ in range(3)]
    for h in hs:
        h.set_precision(_capi.PRECISION_BF16)
        h.set_params(wo, bo); h.set_params(wt, bt, net=1)
    n = hs[0].grad_buffer()[1]
    hs[0].set_target_tau(1.0)
    inject(xq, hs, seeded_gradient(np.random.default_rng(3), n, "spread"))
    for h in hs:
        h.apply_grads(1e-3, 1.0 / 3.0)
    hs[1].updateTargetNetwork()
    hs[2].updateTargetNetwork(1.0)
    env = xq.VecEnv(256, seed=9)
    for _ in range(15):
        env.selfplay_step(None)
    q = [h.q_boards(env, 8100, net=1).cpu().numpy().view(np.uint32) for h in hs]
    for h in hs:
        assert np.array_equal(bits(flat(h, 1)), bits(flat(hs[1]))) and np.array_equal(bits(flat(h)), bits(flat(hs[1])))
    assert np.array_equal(q[0], q[1]) and np.array_equal(q[2], q[1])
    assert np.array_equal(q[1], hs[1].q_boards(env, 8100, net=0).cpu().numpy().view(np.uint32))
    env.close()
    for h in hs:
        h.close()


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_tau_zero_has_the_bits_and_launches_of_never_asked(xq, opt):
    n = 1024
    S = batch(xq, n, 61)
    outs, stats = [], []
    for mode in ("never", "on_then_off", "explicit_zero"):
        d, _, _ = make_net(xq, CFG2_NET, seed=5)
        d.set_optimizer(opt)
        wt, bt = seeded_params(CFG2_NET, 42)
        d.set_params(wt, bt, net=1)
        if mode == "on_then_off":
            d.set_target_tau(0.3); d.set_target_tau(0.0)
        assert d.target_tau() == 0.0
        t0 = flat(d, 1)
        rp = ring(xq, S)
        d.kernel_stats(2)
        for _ in range(3):
            rp.sample(n)
            d.td_grads_replay(rp, n, td_net=1, mode=0)
            d.apply_grads(1e-2, 1.0 / n)
            if mode == "explicit_zero":
                d.updateTargetNetwork(0.0)
        stats.append(launches(d))
        assert np.array_equal(bits(flat(d, 1)), bits(t0))
        outs.append(flat(d))
        rp.close(); d.close()
    assert np.array_equal(bits(outs[0]), bits(outs[1])) and np.array_equal(bits(outs[0]), bits(outs[2]))
    assert stats[0] == stats[1] == stats[2] and "soft_target" not in stats[0]
    assert stats[0]["adam_apply" if opt == "adam" else "sgd_apply"] == 3


def test_tau_outside_the_unit_interval_is_refused_and_what_the_setting_survives(xq, tmp_path):
    from cn_chess_ai_amd import _capi
    d, w, b = make_net(xq, REF_NET, seed=2)
    t = xq.Trainer(xq.TrainerConfig(n_games=16, layer_sizes=REF_NET, replay_capacity=64, minibatch=16))
    for bad in (-0.1, 1.5, float("nan")):
        for name, h in (("xq_dqn_set_target_tau", d.handle), ("xq_dqn_soft_update_target", d.handle), ("xq_trainer_set_target_tau", t._h)):
            with pytest.raises(xq.XqError) as e:
                _capi.call(name, h, bad)
            assert e.value.code == 1, (name, bad)
        with pytest.raises(ValueError):
            d.set_target_tau(bad)
    assert d.target_tau() == 0.0 and t.dqn.target_tau() == 0.0
    _capi.call("xq_dqn_get_target_tau", d.handle, None)                  # the out pointer may be NULL
    d.set_target_tau(0.01)
    path = str(tmp_path / "m.bin")
    d.saveModel(path)
    d.set_optimizer("adam"); d.set_optimizer("sgd"); d.set_grad_clip(0.5); d.set_params(w, b); d.loadModel(path); d.updateTargetNetwork()
    assert d.target_tau() == 0.01
    t.set_target_tau(0.02)
    t.dqn.set_optimizer("adam"); t.dqn.set_grad_clip(0.5); t.dqn.loadModel(path)
    assert t.dqn.target_tau() == 0.02
    for v in (0.0, 1.0):
        d.set_target_tau(v)
        assert d.target_tau() == v
    # refused while a TD step waits for its apply (as set_grad_clip)
    d.set_fused_apply(True)
    n = 8192
    rp = ring(xq, batch(xq, n, 77))
    rp.sample(n)
    d.td_grads_replay(rp, n, td_net=0, mode=0)
    with pytest.raises(xq.XqError) as e:
        d.set_target_tau(0.5)
    assert e.value.code == 2 and "waiting" in str(e.value)
    d.apply_grads(1e-3, 1.0 / n)
    rp.close(); d.close(); t.close()


def test_backpropagate_never_touches_the_target_and_drops_the_fused_form(xq):
    """xq_dqn_backpropagate moves every online parameter and no target parameter whatever tau says; afterwards the nets differ outside
    the TD segments, so the next apply is followed by the whole-buffer kernel and the target's rows >= 96 move too."""
    from cn_chess_ai_amd import _capi
    import test_dqn_gpu as tg
    sizes = REF_NET
    d, _, _ = make_net(xq, sizes, seed=2)
    d.set_target_tau(0.3)
    t0 = flat(d, 1)
    x = tg.one_hot(batch(xq, 1024, 61)[0][:4])
    d.backpropagate(x, np.zeros((4, 8100)), 0.5, 1.0, _capi.BACKPROP_TEXTBOOK)
    assert np.array_equal(bits(flat(d, 1)), bits(t0)) and not np.array_equal(flat(d), t0)
    cov = td_mask(sizes)
    n = d.grad_buffer()[1]
    inject(xq, (d,), seeded_gradient(np.random.default_rng(1), n, "spread"))
    d.kernel_stats(2)
    d.apply_grads(1e-3, 1.0 / 3.0)
    assert launches(d).get("soft_target") == 1
    p, t1 = flat(d), flat(d, 1)
    assert check_step(t0, p, t1, 0.3) <= 1.0 and (t1[~cov] != t0[~cov]).sum() > 0
    d.close()


# ---- 5. the explicit call -----------------------------------------------------------------------------------------------------------
@NETS
def test_explicit_soft_update_of_nets_that_differ_everywhere(xq, sizes):
    """soft_update_target(0.25) whatever the setting says (0 here): every target parameter within the one-step bound, the online net
    untouched, one soft_target launch.  1260-127-129-8100 has 1229659 parameters: three are left for the scalar tail."""
    d = xq.DQN(sizes, seed=1)
    wo, bo = seeded_params(sizes, 41)
    wt, bt = seeded_params(sizes, 42)
    d.set_params(wo, bo); d.set_params(wt, bt, net=1)
    p0, t0 = flat(d), flat(d, 1)
    if sizes == MISALIGNED_NET:
        assert p0.size == 1229659 and p0.size % 4 == 3
    d.kernel_stats(2)
    d.updateTargetNetwork(0.25)
    assert launches(d) == {"soft_target": 1}
    t1 = flat(d, 1)
    worst = check_step(t0, p0, t1, 0.25)
    print("explicit soft update err/bound", sizes, round(worst, 4))
    assert worst <= 1.0 and np.array_equal(bits(flat(d)), bits(p0)) and (t1 != t0).mean() > 0.999
    assert d.target_tau() == 0.0
    # the tail elements moved like the rest
    assert np.abs(t1[-3:].astype(np.float64) - pr.step(t0[-3:], p0[-3:], pr.tau32(0.25))).max() < 1e-8
    d.close()


# ---- 6. the target as the net the TD step reads -------------------------------------------------------------------------------------
def drive(d, S, steps, td_net, n, after=None):
    ys = []
    for i in range(steps):
        Sb, A, R, D, S2 = S[i & 1]
        _, y = d.td_update(Sb, S2, A, R, D, td_net=td_net, mode=0, learning_rate=0.5, grad_scale=1.0 / n)
        ys.append(y.copy())
        if after:
            after(i)
    return ys


@pytest.mark.parametrize("n", [512, 1024])
def test_screening_shadow_follows_a_soft_updated_target(xq, n):
    """td_net = TARGET with XQ_QMAX_SCREENED on 1260-256-256-8100, tau = 0.05, eight steps: the screen keeps its bf16 copy of the
    selecting net's rows >= 96 from step to step and reconverts rows 0..95, which is exactly what the fused soft update changes.
    n = 512: the screen does not engage (see the module docstring) and y equals the XQ_QMAX_FULL twin's bit for bit.  n = 1024: every
    step is screened; y is bit-equal to a screened twin whose target is set before every step by set_params(target, readback) — all 254
    row blocks converted afresh — and within 2e-6 of the full product's."""
    from cn_chess_ai_amd import _capi
    tau, steps = 0.05, 8
    S = [batch(xq, n, 61), batch(xq, n, 62)]
    hs = {}
    for name, mode in (("screened", _capi.QMAX_SCREENED), ("full", _capi.QMAX_FULL), ("refreshed", _capi.QMAX_SCREENED)):
        d, _, _ = make_net(xq, CFG2_NET, seed=8)
        d.set_qmax_mode(mode)
        d.set_target_tau(tau)
        hs[name] = d
    a, r = hs["screened"], hs["refreshed"]
    ya = drive(a, S, steps, _capi.TD_TARGET_NET, n)
    yf = drive(hs["full"], S, steps, _capi.TD_TARGET_NET, n)
    # the refreshed twin: same soft updates (whole-buffer form after the first set_params: same bits), shadow rebuilt every step
    yr = drive(r, S, steps, _capi.TD_TARGET_NET, n, after=lambda i: r.set_params(*r.get_params(1), net=1))
    screened_steps = a.qmax_stats()[0]
    diff_full = max(float(np.abs(x - y).max()) for x, y in zip(ya, yf))
    print("screened target: steps screened", screened_steps, "max |y - y_full|", diff_full)
    assert screened_steps == (steps if n >= 897 else 0) and r.qmax_stats()[0] == screened_steps
    for i in range(steps):
        assert np.array_equal(bits(ya[i]), bits(yr[i])), i
    assert np.array_equal(bits(flat(a, 1)), bits(flat(r, 1))) and np.array_equal(bits(flat(a)), bits(flat(r)))
    if n < 897:
        for i in range(steps):
            assert np.array_equal(bits(ya[i]), bits(yf[i])), i
    else:
        assert diff_full < 2e-6
    assert not np.array_equal(ya[0], ya[2])                              # (same batch, moved target: the targets did change)
    for d in hs.values():
        d.close()


def test_double_dqn_bf16_reads_the_soft_updated_target_and_its_shadow(xq):
    """XQ_TD_DOUBLE under XQ_PRECISION_BF16, three steps with tau = 0.05 (fused form) against a twin with tau = 0 whose target is set
    before every step by set_params(target, readback of the first), which converts every shadow afresh: y bit-equal at every step."""
    from cn_chess_ai_amd import _capi
    n, tau = 512, 0.05
    S = [batch(xq, n, 61), batch(xq, n, 62)]
    a, _, _ = make_net(xq, CFG2_NET, seed=8)
    c, _, _ = make_net(xq, CFG2_NET, seed=8)
    for h in (a, c):
        h.set_precision(_capi.PRECISION_BF16)
    a.set_target_tau(tau)
    a.kernel_stats(2)
    for i in range(3):
        Sb, A, R, D, S2 = S[i & 1]
        _, ya = a.td_update(Sb, S2, A, R, D, td_net=_capi.TD_DOUBLE, mode=0, learning_rate=0.5, grad_scale=1.0 / n)
        _, yc = c.td_update(Sb, S2, A, R, D, td_net=_capi.TD_DOUBLE, mode=0, learning_rate=0.5, grad_scale=1.0 / n)
        assert np.array_equal(bits(ya), bits(yc)), i
        assert np.array_equal(bits(flat(a)), bits(flat(c)))
        c.set_params(*a.get_params(1), net=1)
    assert "soft_target" not in launches(a)
    assert not np.array_equal(flat(a, 1), flat(a)) and np.array_equal(bits(flat(c, 1)), bits(flat(a, 1)))
    a.close(); c.close()


# ---- 7. trainer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cap,minibatch", [(64, 256, 48), (2048, 1 << 15, 2048)])
def test_overlapped_trainer_with_tau_equals_its_sequential_definition(xq, n, cap, minibatch):
    """Trainer.set_target_tau(0.01) with td_net = TARGET and target_sync_interval = 0, 12 iterations, at the game counts of
    tests/test_trainer_gpu.py's overlap test: the overlapped schedule, its sequential definition composed by hand from DQN, VecEnv and
    ReplayBuffer (that test's loop, with DQN.set_target_tau in place of the periodic copy), and the overlapped trainer behind a one-rank
    communicator give bit-identical online and target parameters."""
    import torch
    from cn_chess_ai_amd import dist as xd
    from ring_window_ref import overlap_window
    seed, first, iters, tau, sizes = 99, 7, 12, 0.01, CFG2_NET
    mk = lambda: xq.TrainerConfig(n_games=n, layer_sizes=sizes, learning_rate=0.01, gamma=0.99, epsilon=0.2, replay_capacity=cap,
                                  minibatch=minibatch, td_net=1, backprop_mode=0, target_sync_interval=0, mean_gradient=1, seed=seed,
                                  first_game_id=first, collects_per_update=1, overlap_collect=1)
    t = xq.Trainer(mk())
    w0, b0 = t.dqn.get_params()
    t.set_target_tau(tau)
    assert t.dqn.target_tau() == tau
    t.step(iters)
    got = (flat(t.dqn), flat(t.dqn, 1))
    assert t.counters()["updates"] == iters
    tboards, _ = t.env.get_state()

    tc = xq.Trainer(mk())
    comm = xd.Comm(rank=0, world=1)
    tc.set_comm(comm)
    tc.set_target_tau(tau)
    tc.step(iters)
    assert comm.info()["collectives"] >= iters
    assert np.array_equal(bits(flat(tc.dqn)), bits(got[0])) and np.array_equal(bits(flat(tc.dqn, 1)), bits(got[1]))
    tc.close(); comm.close()

    env = xq.VecEnv(n, seed=seed, first_game_id=first)
    d = xq.DQN(sizes, 0.01, 0.99, seed=1)
    d.set_params(w0, b0); d.updateTargetNetwork()
    d.set_target_tau(tau)
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
    boards, _ = env.get_state()
    assert np.array_equal(boards, tboards)
    assert np.array_equal(bits(flat(d)), bits(got[0])) and np.array_equal(bits(flat(d, 1)), bits(got[1]))
    cov = td_mask(sizes)
    assert (got[1][cov] != np.concatenate([w0, b0]).astype(np.float32)[cov]).sum() > 100 and not np.array_equal(got[0], got[1])
    t.close(); env.close(); d.close(); rp.close()


# ---- the C++ facade -----------------------------------------------------------------------------------------------------------------
def test_facade_soft_update_is_the_c_abi_call(xq):
    """xq::ChessAI::setTargetTau forwards to its network (xq::DQN::targetTau reads it back, setOptimizer and setGradClip leave it, a tau
    outside [0, 1] is std::invalid_argument); xq::DQN::updateTargetNetwork(0.5) gives the bits of xq_dqn_soft_update_target(0.5), moves
    the target to the midpoint within rounding, and updateTargetNetwork(1.0) is the copy."""
    from test_polyak_ref_cpu import build_soft_target_facade_probe
    exe = build_soft_target_facade_probe()
    out = subprocess.run([exe, "7"], check=True, capture_output=True, text=True, timeout=120).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["before"], r["set"], r["after"], r["refused"]) == (0.0, 0.01, 0.01, 3)
    assert r["facade_vs_capi"] == 0.0 and r["moved"] > 1e-3 and r["off_midpoint"] <= 2.0 ** -24 * 0.2 and r["tau_one_is_the_copy"] == 1
