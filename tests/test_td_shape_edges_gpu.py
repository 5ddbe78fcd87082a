"""One TD step at every kernel-selection boundary of xq_dqn.hip against the batched fp64 reference (tests/batch_ref.py) — `pytest -m gpu`.

A TD step is assembled from about thirty kernels that shape predicates pick.  The small-batch tests run the general tile kernel and
single-chunk sums, tests/test_td_full_size_gpu.py whole tiles at 8192 and 16384 samples; the predicates flip in between.  The table of
tests/td_edge_cases.py puts one small case on each side of each of them.  Every case runs ONE step and checks every Q(s,a), every y, the
loss and every parameter with the bounds of batch_ref.TOLERANCES and the exact checks of batch_ref.check_update, and asserts from the
kernel_stats names that the path the case was written for is the one that ran.  Largest err / bound per case on an MI355X:
profiles/NOTES.md ("TD step at the kernel-selection boundaries").
"""
import numpy as np
import pytest

import batch_ref as br
import td_edge_cases as tc
import xqoracle as xo
from test_dqn_gpu import make_net
from test_td_full_size_gpu import selfplay_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


_batches = {}


def batch_of(xq, n, seed):
    """the self-play transitions of (n, seed), as tests/test_td_full_size_gpu.py::run_case draws them; shared by the cases, never written"""
    if (n, seed) not in _batches:
        _batches[(n, seed)] = selfplay_batch(xq, n, seed=1000 + n + seed, plies=20 + (n + seed) % 21, every=7 + seed % 5)
    return _batches[(n, seed)]


def net_of(xq, c):
    """a handle with the case's net, a target net that differs from it, and the case's switches"""
    from cn_chess_ai_amd import _capi
    d, _, _ = make_net(xq, c.sizes, seed=21 + c.seed)
    wt, _ = xo.init_weights(c.sizes, 99 + c.seed)
    bt = np.random.default_rng(98 + c.seed).uniform(-0.05, 0.05, size=xo.nn_counts(c.sizes)[1])
    d.set_params(wt, bt, net=1)
    d.set_qmax_mode(_capi.QMAX_SCREENED if c.sw["qmax"] == "screened" else _capi.QMAX_FULL)
    d.set_l0_derive(c.sw["derive"])
    d.set_fused_apply(c.sw["fused"])
    d.set_td_tail(c.sw["tail"])
    d.set_l0_grad_mode(c.sw["l0grad"])
    return d


def step_against_reference(xq, d, c):
    """One TD step of case c on handle d (at the handle's present precision, which must be c.prec) and in the reference: Q, y, the
    loss, every parameter and the paths.  Returns (err / bound per layer, flipped samples, launches by bracket name)."""
    S, A, R, D, S2 = batch_of(xq, c.n, c.seed)
    w0, b0 = d.get_params()                                   # what the device starts from (fp32 values)
    wt0, bt0 = d.get_params(1)
    d.kernel_stats(2)
    q_dev, y_dev = d.td_update(S, S2, A, R, D, td_net=c.rule, mode=c.mode, learning_rate=c.lr, grad_scale=c.scale)
    launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
    loss_dev = d.last_loss()
    new_w, new_b = d.get_params()
    net = br.Net(c.sizes, w0, b0, c.prec)
    tnet = br.Net(c.sizes, wt0, bt0, c.prec) if c.rule != 0 else None
    f = br.forward(net, S, S2, A, R, D, 0.99, c.rule, c.prec, target=tnet)
    flipped, y_use = br.check_q_y(f, q_dev, y_dev, c.prec)
    loss_ref = br.loss(f, y_use)
    print("loss", loss_dev, loss_ref, "flipped", len(flipped), "bf16 delta / gradient layers", tc.bf16_delta_layers(c), tc.bf16_grad_layers(c))
    assert abs(loss_dev - loss_ref) <= br.LOSS_RTOL[c.prec] * loss_ref, (loss_dev, loss_ref)
    bk = br.backward(net, f, c.mode, c.prec, None, y=y_use, bf16_layers=tc.bf16_delta_layers(c))
    u = br.accumulate(net, f, bk, c.prec, bf16_layers=tc.bf16_grad_layers(c))
    ratios = br.update_ratios(net, u, new_w, new_b, c.lr, c.scale, c.prec)
    print("err/bound", {k: round(v, 4) for k, v in ratios.items()})
    print("launches", launches)
    br.check_update(net, u, f, new_w, new_b, c.lr, c.scale, c.prec)
    for name, ran in tc.expected_paths(c).items():
        assert (launches.get(name, 0) > 0) == ran, (name, ran, launches)
    return ratios, flipped, launches


@pytest.mark.parametrize("name", list(tc.CASES))
def test_td_step_on_a_selection_boundary_matches_the_batched_reference(xq, name):
    c = tc.CASES[name]
    d = net_of(xq, c)
    d.set_precision(c.prec)
    try:
        step_against_reference(xq, d, c)
    finally:
        d.close()


def test_bf16_net_with_an_odd_width_is_refused_and_the_fp32_step_after_it_is_right(xq):
    """1260-127-129-132-8100 switched to bf16: the bf16 products read pairs of elements, so the switch itself refuses odd hidden widths
    (XQ_ERR_INVALID_ARGUMENT) and no kernel of a bf16 step on such a net is ever queued.  The handle stays an fp32 net: its next step
    (the scalar loops of the tile kernel) gives the reference result."""
    from cn_chess_ai_amd import _capi
    c = tc._case("c", "1260-127-129-132-8100", 37)
    assert c.mode == 1
    d = net_of(xq, c)
    try:
        for prec in (_capi.PRECISION_BF16, _capi.PRECISION_BF16_FULL):
            with pytest.raises(_capi.XqError) as e:
                d.set_precision(prec)
            assert e.value.code == 1 and "even" in str(e.value)
        step_against_reference(xq, d, c)
    finally:
        d.close()


@pytest.mark.parametrize("tail", [True, False])
def test_first_hidden_layer_too_wide_for_the_layer0_sums_is_refused_before_the_gradients(xq, tail):
    """1260-1136-64-8100: one accumulator set of 14 x 1136 floats and the sample list need 65664 bytes of LDS, more than a block can
    have, so the step is refused (XQ_ERR_INVALID_ARGUMENT) with the gradient half's other shape check, before its first gradient launch.
    Afterwards no parameter has moved and no step is waiting for its apply (the setters that refuse in that state accept), and a step of
    the widest accepted net, 1260-1132-64-8100, passes."""
    from cn_chess_ai_amd import _capi
    sw = dict(tail=tail, fused=tail)
    c = tc._case("e", "1260-1136-64-8100", 37, **sw)
    d = net_of(xq, c)
    S, A, R, D, S2 = batch_of(xq, c.n, c.seed)
    try:
        before = d.get_params() + d.get_params(1)
        with pytest.raises(_capi.XqError) as e:
            d.td_update(S, S2, A, R, D, td_net=0, mode=c.mode, learning_rate=c.lr, grad_scale=c.scale)
        assert e.value.code == 1 and "layer-0 gradient kernel" in str(e.value)
        d.set_optimizer("adam")
        d.set_grad_clip(1.0)
        d.set_precision(_capi.PRECISION_F32)
        for got, want in zip(d.get_params() + d.get_params(1), before):
            assert np.array_equal(got, want)
    finally:
        d.close()
    c = tc._case("e", "1260-1132-64-8100", 37, **sw)
    d = net_of(xq, c)
    try:
        step_against_reference(xq, d, c)
    finally:
        d.close()
