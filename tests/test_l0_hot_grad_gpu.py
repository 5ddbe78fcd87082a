"""The layer-0 gradient of the fused launch: packed hot rows on the matrix pipe, cold rows summed from occurrence lists
(csrc/xq_l0grad.hip.h, csrc/xq_l0hot.h).  No result may depend on which rows the table calls hot, so one TD step is taken on
  * play   — positions of the reference trace: no cold row occurs, every cold row of the gradient must be written as +0.0;
  * random — a piece of a uniformly random kind on every square of every board: all 1260 rows occur (asserted), the first and last
             packed row of every row group, the rows that share a tile with padding and row 1259 among them;
  * cold   — boards that hold pieces on cold rows only: the matrix-pipe blocks multiply nothing but zeros
at the smallest shapes where the kernels can go wrong: H = 64 (two column blocks; one hidden layer: the selector pass is a launch of
its own) and H = 256 (two hidden layers: it rides in fused launch 1); n = 256 (the first size on this route), 300 (a partial stage
of 64 samples), 1025 (a second chunk that holds one sample).
Each step is compared with the batched fp64 reference (tests/batch_ref.py, the restatement of xqo_nn_accum_grad; at H = 64, n = 256 its
layer-0 gradient is compared with xo.nn_accum_grad sample by sample) within the bound tests/test_dqn_gpu.py applies to the matrix-pipe
form, and with the segmented sums (set_l0_grad_mode(0)): everything outside layer 0 bit-identical; hot rows within that test's
HIP-vs-HIP bound (two ulps of the stored weight, 8e-9); cold rows within what two fp32 summation orders of the same m terms can
differ by, lr * scale * 2 (m - 1) 2^-24 sum |delta| (Higham, Accuracy and Stability, eq. 4.4, once per order), plus those two ulps."""
import numpy as np
import pytest

import batch_ref as br
import xqoracle as xo
from l0_hot_ref import hot_mask_rows, load_table
from test_dqn_gpu import CFG2_NET, make_net, one_hot, transitions, valid_indices

pytestmark = pytest.mark.gpu

NETS = {64: [1260, 64, 8100], 256: CFG2_NET}
LR = 0.05


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


@pytest.fixture(scope="module")
def trace(golden_dir):
    import os
    return np.load(os.path.join(golden_dir, "ref_trace.npz"))


def batch(trace, kind, n):
    """(S, S2, A, R, D) of n transitions of one board set"""
    if kind == "play":
        S, A, R, D, S2 = transitions(trace, valid_indices(trace, n, seed=6))
        return np.asarray(S, np.uint8), np.asarray(S2, np.uint8), np.asarray(A, np.int32), (np.asarray(R) / 1000.0).astype(np.float32), np.asarray(D, np.uint8)
    rng = np.random.default_rng(1000 + n)
    if kind == "random":
        S = rng.integers(1, 15, size=(n, 90), dtype=np.uint8)
    else:
        hot = hot_mask_rows(load_table()).reshape(90, 14)
        S = np.zeros((n, 90), np.uint8)
        for s in range(90):
            cold = np.nonzero(~hot[s])[0] + 1
            assert len(cold) >= 4
            S[:, s] = np.where(rng.random(n) < 0.35, rng.choice(cold, size=n), 0)
    S2 = S[rng.permutation(n)]
    return (S, S2, rng.integers(0, 90, size=n).astype(np.int32), rng.uniform(-0.5, 0.5, size=n).astype(np.float32), (rng.random(n) < 0.1).astype(np.uint8))


@pytest.mark.parametrize("kind", ["play", "random", "cold"])
@pytest.mark.parametrize("n", [256, 300, 1025])
@pytest.mark.parametrize("H", [64, 256])
def test_hot_rows_on_the_matrix_pipe_cold_rows_from_their_lists(xq, trace, H, n, kind):
    sizes = NETS[H]
    S, S2, A, R, D = batch(trace, kind, n)
    hot = hot_mask_rows(load_table())
    x = one_hot(S)
    occurs = x.any(axis=0)
    if kind == "play":
        assert not occurs[~hot].any()
    elif kind == "random":
        assert occurs.all()
    else:
        assert occurs[~hot].any() and not occurs[hot].any()
    scale = 1.0 / n
    outs = []
    for mode in (0, 1):
        d, w, b = make_net(xq, sizes, seed=9)
        d.set_l0_grad_mode(mode)
        d.td_update(S, S2, A, R, D, td_net=0, mode=0, learning_rate=LR, grad_scale=scale)
        outs.append(d.get_params())
        d.close()
    (w0, b0), (w1, b1) = outs
    n0 = 1260 * H
    assert np.array_equal(w0[n0:], w1[n0:]) and np.array_equal(b0, b1)
    assert not np.array_equal(w1[:n0], w[:n0])
    # the fp64 reference
    net = br.Net(sizes, w.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64))
    f = br.forward(net, S, S2, A, R, D, 0.99, 0)
    u = br.accumulate(net, f, br.backward(net, f, 0))
    for got_w, got_b in outs:
        ratios = br.check_update(net, u, f, got_w, got_b, LR, scale, br.PRECISION_F32)
    print(f"H={H} n={n} {kind}: ratios {ratios}")
    # against the segmented sums, row by row ([H][1260]: a row of gW0^T is a column here)
    diff = np.abs(w0[:n0] - w1[:n0]).reshape(H, 1260)
    m = x.sum(axis=0)
    order = LR * scale * 2.0 * np.maximum(m - 1.0, 0.0)[None, :] * 2.0 ** -24 * u.T[0]
    print(f"  vs segmented sums: hot {diff[:, hot].max():.3g}, cold {diff[:, ~hot].max():.3g} (order term <= {order[:, ~hot].max():.3g})")
    assert diff[:, hot].max() <= 8e-9
    assert np.all(diff[:, ~hot] <= order[:, ~hot] + 8e-9)
    assert np.array_equal(w1[:n0].reshape(H, 1260)[:, ~occurs], np.asarray(w, np.float32).astype(np.float64)[:n0].reshape(H, 1260)[:, ~occurs])
    if H == 64 and n == 256:
        # batch_ref's layer-0 gradient against the oracle's own, sample by sample
        wf, bf = net_params(net, w, b)
        gw, gb = np.zeros_like(wf), np.zeros_like(bf)
        for s, a, r, dn, s2 in zip(S, A, R, D, S2):
            xs = xo.state_repr(xo.board_from(s))
            tq = xo.td_target(sizes, wf, bf, xs, xo.state_repr(xo.board_from(s2)), int(a), float(r), int(dn), 0.99)
            xo.nn_accum_grad(sizes, wf, bf, xs, tq, 0, gw, gb)
        ref = gw[:n0].reshape(H, 1260)
        assert np.abs(ref - u.gW[0]).max() <= 1e-9 * max(np.abs(ref).max(), 1e-30)


def net_params(net, w, b):
    """the fp32-rounded parameters the device holds, as the oracle's flat fp64 arrays"""
    return (np.ascontiguousarray(np.asarray(w, np.float32).astype(np.float64)), np.ascontiguousarray(np.asarray(b, np.float32).astype(np.float64)))
