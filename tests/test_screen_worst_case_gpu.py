"""The screened max pass on inputs that push the true maximum to the edge of its candidate window — `pytest -m gpu`.

Every other screen test draws its inputs at random, and random bf16 rounding errors stay 10-30 times below the bound B: a window of B
instead of 2B, a bound from the wrong sample's norm or a lost row-norm slot would pass them all.  The cases of tests/screen_worst_cases.py
(construction: tests/screen_ref.py) put the true maximum 0.84 .. 0.87 of the way down the 2B window, behind a rival row that
the bf16 product ranks FIRST; tests/test_screen_ref_cpu.py proves that on the CPU and that each such defect loses the maximum by ten bars.

Per case, on a fresh handle: three screened steps at learning rate 0 (slot parities 0, 1, 0; the bf16 shadow of rows >= 96 is kept from the
second on) give the same bits; they match a step with the full fp32 product within 2e-6 and fp64 within 2e-6 + gamma * 6e-6 * sum_k |W_j*k a_k|
(tanh_hidden's documented relative error, xq_gemm.hip.h, carried through the winning row); the candidate counters of every step are exactly
the model's (two single groups per sample, or one whole group where the two rows share a group), which is what shows that the case was not
vacuous on the device.  Largest |y - ref| per family on an MI355X: profiles/NOTES.md ("Screened max pass on worst-case inputs").
"""
import numpy as np
import pytest

import screen_ref as sr
import screen_worst_cases as wc
from td_edge_cases import reference_mode_defined

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def screened_step(d, c, bt, R, D, A):
    """one screened step: (y, candidate groups, whole groups, launches by bracket name)"""
    before = d.qmax_stats()
    d.kernel_stats(2)
    _, y = d.td_update(bt.boards, bt.boards, A, R, D, td_net=c.td_net, mode=0 if reference_mode_defined(bt.sizes) else 1,
                       learning_rate=0.0, grad_scale=1.0)
    launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
    after = d.qmax_stats()
    assert after[0] - before[0] == 1 and after[1] - before[1] == c.n
    return y.copy(), after[2] - before[2], after[3] - before[3], launches


@pytest.mark.parametrize("name", list(wc.CASES))
def test_screened_maximum_at_the_edge_of_the_candidate_window(xq, name):
    from cn_chess_ai_amd import _capi
    c = wc.CASES[name]
    bt = sr.build(c)
    n = c.n
    R = ((np.arange(n) % 5 - 2) / 64.0).astype(np.float32)
    D = np.zeros(n, np.uint8)
    A = (np.arange(n) * 7 % 90).astype(np.int32)
    want = R.astype(np.float64) + sr.GAMMA * np.tanh(bt.z.max(axis=1))[bt.cls]
    bar = sr.y_bar(bt)[bt.cls]
    pairs, whole = wc.expected_counts(c)
    d = xq.DQN(bt.sizes, 0.001, 0.99, seed=1)
    try:
        # the construction on the net that selects, the decoy (output weights halved: another maximum) on the other one
        d.set_params(bt.w if c.td_net == 0 else bt.w_decoy, bt.b, net=0)
        d.set_params(bt.w if c.td_net == 1 else bt.w_decoy, bt.b, net=1)
        d.set_td_tail(c.tail)
        d.set_refine_stage(0)
        if c.huber:
            d.set_td_loss("huber", 0.03125)
        d.set_qmax_mode(_capi.QMAX_SCREENED)
        ys = []
        for step in range(3):
            y, p, w, launches = screened_step(d, c, bt, R, D, A)
            print(name, "step", step, "pairs", p, "whole", w, "max |y - ref| / bar", (np.abs(y - want) / bar).max(), "max |y - ref|",
                  np.abs(y - want).max())
            assert launches.get("gemm_qmax_screen", 0) == 1 and launches.get("qmax_refine", 0) == 1, launches
            assert launches.get("gemm_qmax_rowmax", 0) == 0, launches
            assert (p, w) == (pairs * n, whole * n)
            ys.append(y)
        assert np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2])
        assert (np.abs(ys[0] - want) < bar).all(), (np.abs(ys[0] - want) / bar).max()
        if c.huber:                                      # the loss shapes the delta, never the target
            d.set_td_loss("squared")
            y_sq, p, w, _ = screened_step(d, c, bt, R, D, A)
            assert np.array_equal(y_sq, ys[0]) and (p, w) == (pairs * n, whole * n)
        if wc.one_group(c):                              # the popular whole group through LDS where the launch has room: the same bits
            d.set_refine_stage(1)
            y_st, p, w, _ = screened_step(d, c, bt, R, D, A)
            assert np.array_equal(y_st, ys[0]) and (p, w) == (pairs * n, whole * n)
        d.set_qmax_mode(_capi.QMAX_FULL)
        d.kernel_stats(2)
        _, y_full = d.td_update(bt.boards, bt.boards, A, R, D, td_net=c.td_net, mode=0 if reference_mode_defined(bt.sizes) else 1,
                                learning_rate=0.0, grad_scale=1.0)
        launches = {s["name"]: s["launches"] for s in d.kernel_stats(0)}
        assert launches.get("gemm_qmax_rowmax", 0) >= 1 and launches.get("gemm_qmax_screen", 0) == 0, launches
        print(name, "max |y_screened - y_full|", np.abs(ys[0] - y_full).max(), "max |y_full - ref| / bar", (np.abs(y_full - want) / bar).max())
        assert np.abs(ys[0] - y_full).max() < sr.Y_BAR
        assert (np.abs(y_full - want) < bar).all()
    finally:
        d.close()


def test_a_td_step_refuses_a_1024_wide_last_hidden_layer(xq):
    """Why the widest case of the table is 960: the screen's plan takes K <= 1024, but the output-gradient kernel's 16 rows of the last
    hidden layer beside its sample list need more than 64 KB of LDS at 1024, so the step is refused (XQ_ERR_INVALID_ARGUMENT) whatever
    the max pass.  K = 1024 goes through the CPU model only (screen_worst_cases.CPU_ONLY)."""
    from cn_chess_ai_amd import _capi
    c = next(iter(wc.CPU_ONLY.values()))
    bt = sr.build(c)
    d = xq.DQN(bt.sizes, 0.001, 0.99, seed=1)
    try:
        d.set_params(bt.w, bt.b, net=0)
        d.set_qmax_mode(_capi.QMAX_SCREENED)
        z = np.zeros(c.n)
        with pytest.raises(_capi.XqError) as e:
            d.td_update(bt.boards, bt.boards, z.astype(np.int32), z.astype(np.float32), z.astype(np.uint8), td_net=0, mode=0,
                        learning_rate=0.0, grad_scale=1.0)
        assert e.value.code == 1 and "output-gradient kernel" in str(e.value)
    finally:
        d.close()
