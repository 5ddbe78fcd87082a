"""After every kind of parameter write, every copy derived from the parameters is current (the table of params_written in xq_dqn.hip):
the screening shadow of output rows >= 96 and the select chain's kept layer-0 sums.

Each case primes both copies for the net about to be written, writes, and then compares with what cannot be stale: a screened TD step
against the same step of a fresh handle that received both nets through get_params -> set_params (same launches, same inputs: the same
bits unless the shadow differs), and the select chain against the direct gather (the first call after a write of the online net is a full
sum in the direct gather's order: the same bits).

What is written has to show in a copy that was kept by mistake.  The screen reads the biases themselves and refines every candidate
exactly, so a stale shadow only shows when the WEIGHTS of a row >= 96 carry it to the top: its stale bf16 row then leaves it below the
candidates.  The nets here have last hidden activations near tanh(0.5) for every unit and sample (base_net), so a row of equal positive
weights wins everywhere; output 8099, a row the TD rule never touches, receives such weights.  Layer 0 moves too, for the kept sums."""
import numpy as np
import pytest

from test_dqn_gpu import CFG2_NET, _selfplay_transitions, make_net, one_hot

pytestmark = pytest.mark.gpu

N = 1024                 # screening needs 8100 outputs on 128-row tiles that fill the chip twice: n >= 897; width 256: screen_top2_kernel
ONLINE, TARGET = 0, 1
L0, H1, H2, _ = CFG2_NET


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


@pytest.fixture(scope="module")
def batch(xq):
    S, S2, A, R, D = _selfplay_transitions(xq, N)
    return S, S2, A, R, D


def base_net(xq):
    """make_net's net with the biases of the last hidden layer raised by 0.5, in both nets: a_k = tanh(0.5 +- 0.1) = 0.46 for every unit of
    every sample.  An output row of random weights in +-0.05 then has z ~ N(b, 0.21): the largest of 8100 is about 0.8, tanh 0.66."""
    d, w, b = make_net(xq, CFG2_NET, seed=8)
    b[H1:H1 + H2] += 0.5
    d.set_params(w, b)
    d.updateTargetNetwork()
    return d, w, b


def written_params(w, b):
    """The net a write installs: row 8099 of the output layer = 0.1 everywhere, z = 0.1 * 256 * 0.46 = 11.8 (half of it after a blend with
    tau = 0.5), tanh = 1 to five digits; and layer 0 moves (weights and biases), so sums kept from the old layer 0 are wrong by far more
    than a summation order."""
    w2, b2 = w.copy(), b.copy()
    w2[-H2:] = 0.1
    w2[:L0 * H1] *= 1.5
    b2[:H1] += 0.02
    return w2, b2


def screened_step(d, batch, td_net):
    """One screened TD step with a zero step size: (Q(s,a), y), and the proof that it screened."""
    before = d.qmax_stats()[0]
    qsa, y = d.td_update(*batch, td_net=td_net, mode=0, learning_rate=0.0, grad_scale=1.0)
    assert d.qmax_stats()[0] == before + 1
    return qsa.copy(), y.copy()


def write_set_params(net):
    def write(xq, d, w, b, tmp_path, batch):
        d.set_params(*written_params(w, b), net=net)
    return write


def write_load_model(xq, d, w, b, tmp_path, batch):
    g = xq.DQN(CFG2_NET, 0.001, 0.99, seed=8)
    g.set_params(*written_params(w, b))
    g.saveModel(tmp_path / "written.bin")
    g.close()
    d.loadModel(tmp_path / "written.bin")


def write_update_target(tau):
    def write(xq, d, w, b, tmp_path, batch):
        d.updateTargetNetwork(tau)
    return write


def write_backpropagate(xq, d, w, b, tmp_path, batch):
    # dense targets = the net's own outputs (no delta) except output 8099, asked to be 2.5 higher: its bias moves by lr * 4 * 2.5 * (1 - q^2)
    # = 0.19 and each of its weights by 0.46 times that, so z_8099 rises by 0.19 * (1 + 256 * 0.46^2) = 10 — all but 0.19 of it through the
    # weights, far past the bf16 bound of the screen; the delta it sends down moves every layer below a little
    x = one_hot(batch[0][:4])
    t = d.getQValues(x)
    t[:, 8099] += 2.5
    d.backpropagate(x, t, learning_rate=0.02, grad_scale=1.0, mode=1)


def write_apply(tau):
    def write(xq, d, w, b, tmp_path, batch):
        d.td_update(*batch, td_net=TARGET if tau else ONLINE, mode=0, learning_rate=0.05, grad_scale=1.0 / N)
    return write


# (name, the net the write rewrites, the write, whether it moves the maximum to row 8099, tau set on the handle)
CASES = [("set_params_online", ONLINE, write_set_params(ONLINE), True, 0.0),
         ("set_params_target", TARGET, write_set_params(TARGET), True, 0.0),
         ("load_model", ONLINE, write_load_model, True, 0.0),
         ("update_target", TARGET, write_update_target(None), True, 0.0),
         ("update_target_tau", TARGET, write_update_target(0.5), True, 0.0),
         ("backpropagate", ONLINE, write_backpropagate, True, 0.0),
         # controls: the TD rule moves rows 0..95 only (the kept rows of the shadow stay valid), and layer 0 (the kept sums do not)
         ("apply_grads", ONLINE, write_apply(0.0), False, 0.0),
         ("apply_grads_fused_soft", TARGET, write_apply(0.5), False, 0.5)]


@pytest.mark.parametrize("name,net,write,moves_max,tau", CASES, ids=[c[0] for c in CASES])
def test_derived_copies_are_current_after(xq, batch, tmp_path, name, net, write, moves_max, tau):
    from cn_chess_ai_amd import _capi
    d, w, b = base_net(xq)
    S, S2, A, R, D = batch
    if name.startswith("update_target"):
        d.set_params(*written_params(w, b), net=ONLINE)          # what the target is about to receive; the target keeps (w, b)
    if tau:
        d.set_target_tau(tau)                                    # in step behind make_net's updateTargetNetwork: the fused form
    env = xq.VecEnv(N, seed=17)
    for _ in range(20):
        env.selfplay_step(None)
    # 1. prime: the shadow holds rows >= 96 of the net about to be written, the select chain's kept sums are live
    d.set_qmax_mode(_capi.QMAX_SCREENED)
    d.set_l0_derive(True)
    _, y_before = screened_step(d, batch, net)
    for _ in range(3):
        d.select_q(env)
        env.selfplay_step(None)
    # 2. write
    write(xq, d, w, b, tmp_path, batch)
    # 4. (before step 3, whose apply drops the kept sums itself) the select chain sums layer 0 in full again after a write of the online net
    if net == ONLINE:
        assert np.array_equal(d.select_q(env).cpu().numpy(), d.q_boards(env, 96).cpu().numpy())
    # 3. a screened step sees the written net: the same bits as on a fresh handle with the same two nets (taken before the step: with a
    #    tau set, its apply blends the target again)
    f = xq.DQN(CFG2_NET, 0.001, 0.99, seed=8)
    for k in (ONLINE, TARGET):
        f.set_params(*d.get_params(k), net=k)
    f.set_qmax_mode(_capi.QMAX_SCREENED)
    f.set_l0_derive(True)
    qsa, y = screened_step(d, batch, net)
    qsa_f, y_f = screened_step(f, batch, net)
    live = D == 0                                                # y = r + 0.99 max_a' Q(s', a')
    qmax_before, qmax = ((y_before - R)[live] / 0.99, (y - R)[live] / 0.99)
    print(name, "max_a' Q(s',a') before the write: median %.4f, largest %.4f; after: median %.4f, smallest %.4f | differing y: %d of %d"
          % (np.median(qmax_before), qmax_before.max(), np.median(qmax), qmax.min(), (y.view(np.uint32) != y_f.view(np.uint32)).sum(), N))
    if moves_max:                                                # the write was not tame: the maximum moved to row 8099 nearly everywhere
        assert (qmax_before < 0.9).mean() > 0.9 and (qmax > 0.999).mean() > 0.9
    assert np.array_equal(qsa.view(np.uint32), qsa_f.view(np.uint32))
    assert np.array_equal(y.view(np.uint32), y_f.view(np.uint32))
    env.close(); d.close(); f.close()
