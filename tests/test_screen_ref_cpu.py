"""CPU checks of tests/screen_ref.py and tests/screen_worst_cases.py (not gpu): the constructed inputs really sit at the edge of the
screen's candidate window, the intact model keeps the true maximum there, and every damaged model loses it by at least ten times the bar
tests/test_screen_worst_case_gpu.py holds the device to.  Measured depths: profiles/NOTES.md ("Screened max pass on worst-case inputs").
"""
import numpy as np
import pytest

import screen_ref as sr
import screen_worst_cases as wc

SEEDS = (None, 1, 2, 3)                  # the intended activations, then three draws of tanh_hidden's documented error
NAMES = wc.constructions()


@pytest.fixture(scope="module", params=NAMES)
def built(request):
    c = wc.case(request.param)
    return c, sr.build(c)


def lost(bt, s):
    """per class: what a target loses when the model returns s.zmax, in units of the case's bar"""
    return sr.GAMMA * (np.tanh(bt.z.max(axis=1)) - np.tanh(s.zmax)) / sr.y_bar(bt)


def model(c, bt, damage=None, seed=None):
    A = bt.a if seed is None else sr.jittered(bt.a, seed)
    return sr.screen(bt.W, bt.bout, A, sr.na_from_bf16(c), damage)


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20, -0.3, 0.0, 2.0 ** -130])
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 1.0, -0.30078125, 0.0, 2.0 ** -130])
    assert np.array_equal(sr.bf16_rne(x), want)
    r = np.random.default_rng(0).standard_normal(4096)
    q = sr.bf16_rne(r)
    assert (np.abs(q - r) <= 2.0 ** -8 * np.abs(r)).all() and np.array_equal(sr.bf16_rne(q), q)


def test_groups_partition_the_rows():
    rows = sr.group_rows(sr.NO)
    assert rows.shape == (254, 32) and np.array_equal(np.sort(rows.ravel()), np.arange(254 * 32))
    assert sr.group_of(200) == sr.group_of(201) and sr.group_of(8099) == sr.group_of(8064) == 252
    for a, b in ((4321, 17), (8099, 8068), (0, 95), (40, 70)):
        assert sr.group_of(a) != sr.group_of(b)
    assert {wc.one_group(c) for c in wc.CASES.values()} == {True, False}


def test_the_table_covers_what_it_names():
    cs = list(wc.CASES.values())
    assert {c.Hl for c in cs} == {128, 256, 512, 960} and {c.n for c in cs} == {897, 1024, 1100}
    for Hl in (128, 256, 512, 960):
        at = [c for c in cs if c.Hl == Hl]
        assert {c.net for c in at} == {"gather", "product"} and {c.td_net for c in at} == {0, 1} and any(c.biased for c in at)
        assert {c.n for c in at if c.family == "a"} >= {1024, 1100}
    at = [c for c in cs if c.Hl == 256]
    assert {(c.jstar, c.rival) for c in at} >= {p for pair in wc.PAIRS for p in (pair, pair[::-1])}
    assert {(c.tail, c.huber, c.n) for c in at if c.family == "a"} == {(t, h, n) for t, h in ((True, False), (True, True), (False, False))
                                                                       for n in (897, 1024, 1100)}
    assert all(c.low_static == ({c.jstar, c.rival} == {40, 70}) for c in cs)


@pytest.mark.parametrize("net", ["gather", "product"])
def test_the_parameter_vectors_produce_the_intended_activations(net):
    """a plain fp64 forward pass of the builder's flat parameter vectors on its boards: the last hidden layer holds the intended
    activations of each sample's class and the output layer the z the tests compare against"""
    c = wc._case("t", 128, 40, net, (200, 201), biased=True)
    bt = sr.build(c)
    x = np.zeros((c.n, 1260))
    for i, bd in enumerate(bt.boards):
        for s in np.nonzero(bd)[0]:
            x[i, s * 14 + bd[s] - 1] = 1.0
    assert (x.sum(axis=1) == 3).all() and set(bt.cls) == set(range(sr.N_CLASSES))
    wo = bo = 0
    for fan_in, fan_out in zip(bt.sizes[:-2], bt.sizes[1:-1]):
        x = np.tanh(x @ bt.w[wo:wo + fan_in * fan_out].reshape(fan_out, fan_in).T + bt.b[bo:bo + fan_out])
        wo += fan_in * fan_out
        bo += fan_out
    assert np.abs(x / bt.a[bt.cls] - 1.0).max() < 1e-12
    W = bt.w[wo:].reshape(sr.NO, c.Hl)
    assert wo + sr.NO * c.Hl == len(bt.w) and bo + sr.NO == len(bt.b)
    assert np.array_equal(sr.f32(W), bt.W) and np.array_equal(bt.w_decoy[wo:], 0.5 * bt.w[wo:]) and np.array_equal(bt.w_decoy[:wo], bt.w[:wo])
    assert np.abs(x @ W.T + bt.b[bo:] - bt.z[bt.cls]).max() < 1e-9


def test_the_true_maximum_sits_deep_in_the_window_and_the_intact_model_keeps_it(built):
    c, bt = built
    assert (bt.z.argmax(axis=1) == c.jstar).all()
    second = np.sort(bt.z, axis=1)[:, -2]
    assert np.array_equal(second, bt.z[:, c.rival])
    assert np.abs(bt.z[:, c.jstar]).max() < 0.1                      # near z = 0, where tanh' ~ 1
    pairs, whole = wc.expected_counts(c)
    for seed in SEEDS:
        d = sr.depth(c, seed, bt)
        print(wc.name_of(c), "seed", seed, "depth", d.min(), d.max())
        assert d.min() >= 0.8 and d.max() < 1.0
        s = model(c, bt, seed=seed)
        assert (s.zt.argmax(axis=1) == c.rival).all()                # the screen's own arg-max is the WRONG row
        assert all(c.jstar in k for k in s.kept)
        A = bt.a if seed is None else sr.jittered(bt.a, seed)
        assert np.array_equal(s.zmax, (sr.f32(A) @ bt.W.T + bt.bout).max(axis=1))
        assert (s.pairs == pairs).all() and (s.whole == whole).all()


def test_the_gap_is_visible_at_the_bar(built):
    c, bt = built
    gap = sr.GAMMA * (np.tanh(bt.z[:, c.jstar]) - np.tanh(bt.z[:, c.rival]))
    print(wc.name_of(c), "gap / bar", (gap / sr.y_bar(bt)).min())
    assert (gap >= 10.0 * sr.y_bar(bt)).all()


def test_a_window_of_one_bound_loses_the_maximum(built):
    c, bt = built
    for seed in SEEDS:
        assert (lost(bt, model(c, bt, "half_window", seed)) >= 10.0).all()


def test_the_sensitivity_to_the_size_of_the_bound(built):
    """A bound that is too small loses the maximum once factor * (1 + 2^-5) falls below the depth.  The cases sit at depth 0.84 .. 0.87:
    eps * 0.9 (and anything above 0.85) still keeps the maximum, eps * 0.8 and eps * 0.5 (u in place of 2u) lose it.  The cases therefore
    detect a bound that is more than about 15 % too small."""
    c, bt = built
    d = sr.depth(c, None, bt)
    assert 0.8 * sr.THR_REEVAL < d.min() and d.max() < 0.9 * sr.THR_REEVAL
    assert (lost(bt, model(c, bt, "eps_0.9")) == 0.0).all()
    for f in ("eps_0.8", "eps_0.5"):
        assert (lost(bt, model(c, bt, f)) >= 10.0).all()


def test_the_norm_of_the_neighbouring_sample_loses_the_maximum(built):
    """classes alternate sample by sample and class q ^ 1 has half or twice the scale: the sample with the larger one gets half its bound"""
    c, bt = built
    ls = lost(bt, model(c, bt, "neighbour"))
    assert (ls[0::2] >= 10.0).all() and (ls[1::2] == 0.0).all()


@pytest.mark.parametrize("name", [n for n in NAMES if wc.case(n).low_static])
def test_row_norms_of_the_static_rows_alone_lose_the_maximum(name):
    """aimed at the (40, 70) family: rows >= 96 have a tenth of the norm"""
    c = wc.case(name)
    bt = sr.build(c)
    assert np.sqrt((bt.W[sr.DYN_ROWS:] ** 2).sum(axis=1)).max() < 0.11 * np.linalg.norm(bt.W[c.jstar])
    assert (lost(bt, model(c, bt, "static_only")) >= 10.0).all()


@pytest.mark.parametrize("name", [n for n in NAMES if wc.one_group(wc.case(n))])
def test_without_the_whole_group_rule_the_maximum_is_lost(name):
    """aimed at the families whose two rows share a group"""
    c = wc.case(name)
    bt = sr.build(c)
    s = model(c, bt, "no_whole")
    assert all(k == [c.rival] for k in s.kept)
    assert (lost(bt, s) >= 10.0).all()


def test_the_intact_model_finds_the_maximum_of_random_nets():
    """near-tied rows (one base row + perturbations of a bf16 rounding step, so that the screen's arg-max is mostly wrong), plain random
    rows, biases, several widths and output counts with a ragged last chunk: 240 nets x 4 samples"""
    rng = np.random.default_rng(5)
    wrong = 0
    for t in range(240):
        no, K = int(rng.integers(97, 700)), int(rng.choice([64, 128, 192]))
        A = rng.uniform(-1, 1, (4, K)) * 2.0 ** -rng.integers(0, 4)
        if t % 3:
            W = rng.uniform(-0.05, 0.05, K)[None, :] * (1.0 + 2.0 ** -9 * rng.standard_normal((no, K)))
        else:
            W = rng.uniform(-0.05, 0.05, (no, K))
        b = rng.uniform(-0.3, 0.3, no) * (t % 2)
        s = sr.screen(W, b, A, bool(t & 4))
        assert np.array_equal(s.zmax, s.z.max(axis=1))
        wrong += int((s.zt.argmax(axis=1) != s.z.argmax(axis=1)).sum())
    assert wrong > 200
