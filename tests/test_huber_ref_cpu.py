"""CPU checks of the Huber TD loss's reference (not gpu): tests/huber_ref.py is torch.nn.functional.huber_loss and its autograd
gradient, kappa = inf gives the weights batch_ref uses today, and header, ctypes table and library agree on the new entry points."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import batch_ref as br
import huber_ref as hr
from test_arena_cpu import gxx, BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_dqn_set_td_loss", "xq_dqn_get_td_loss", "xq_dqn_td_error_stats")


def seeded_errors(seed, n=4096):
    """|e| spread over 1e-6 .. 1e4, both signs, plus exact zeros and values exactly at +-kappa candidates"""
    rng = np.random.default_rng(seed)
    e = 10.0 ** rng.uniform(-6, 4, size=n) * rng.choice([-1.0, 1.0], size=n)
    e[:8] = [0.0, 0.1, -0.1, 1.0, -1.0, 5.0, -5.0, 0.0]
    q = np.tanh(rng.uniform(-2, 2, size=n))
    return q, q - e, e


class FakeForward:
    def __init__(self, q, y):
        self.q, self.y, self.n, self.live = q, y, len(q), np.ones(len(q), bool)


@pytest.mark.parametrize("kappa", [0.1, 1.0, 5.0])
def test_huber_ref_is_torch_huber_loss_and_its_gradient(kappa):
    import torch
    q, y, e = seeded_errors(int(kappa * 10))
    f = FakeForward(q, y)
    tq = torch.tensor(q, dtype=torch.float64, requires_grad=True)
    tl = torch.nn.functional.huber_loss(tq, torch.tensor(y, dtype=torch.float64), reduction="sum", delta=kappa)
    tl.backward()
    g = tq.grad.numpy()
    assert abs(hr.loss(f, kappa) - float(tl.detach())) <= 1e-12 * float(tl.detach())
    assert np.abs(hr.clamp(e, kappa) - g).max() <= 1e-12
    # the weights form: e * factor == dL/dq, the factor is exactly 1 in the quadratic part and at e = 0
    w = hr.weights(f, kappa)
    assert np.abs(w * (q - y) - g).max() <= 1e-12 * max(1.0, kappa)
    assert np.array_equal(w[np.abs(q - y) <= kappa], np.ones(int((np.abs(q - y) <= kappa).sum())))
    assert (np.abs(e) > kappa).sum() > 100 and (np.abs(e) <= kappa).sum() > 100
    # importance weights multiply the factor
    iw = np.random.default_rng(1).uniform(0.1, 1.0, size=len(q))
    assert np.array_equal(hr.weights(f, kappa, iw), iw * w)


def test_kappa_inf_gives_the_weights_batch_ref_uses_today():
    q, y, _ = seeded_errors(3)
    f = FakeForward(q, y)
    assert np.array_equal(hr.weights(f, math.inf), np.ones(f.n))
    iw = np.random.default_rng(2).uniform(0.1, 1.0, size=f.n)
    assert np.array_equal(hr.weights(f, math.inf, iw), iw)
    assert hr.loss(f, math.inf) == float(np.sum(0.5 * np.abs(q - y) ** 2))
    assert abs(hr.loss(f, math.inf) - br.loss(f)) <= 1e-15 * br.loss(f)


def test_stats_restate_the_record():
    q, y, _ = seeded_errors(5, n=1000)
    live = np.ones(1000, bool); live[::7] = False
    e = (q.astype(np.float32) - y.astype(np.float32)).astype(np.float64)[live]
    s = hr.stats(q, y, live, 1.0)
    assert s["live"] == int(live.sum()) and s["max_abs"] == np.abs(e).max() and s["linear"] == int((np.abs(e) > 1.0).sum())
    assert abs(s["mean_abs"] - np.abs(e).mean()) <= 1e-15 * s["mean_abs"]
    sq = hr.stats(q, y, live, math.inf)
    assert sq["linear"] == 0 and abs(sq["mean_loss"] - np.mean(0.5 * e * e)) <= 1e-15 * sq["mean_loss"]
    assert hr.stats(q, y, np.zeros(1000, bool), 1.0) == dict(live=0, mean_abs=0.0, max_abs=0.0, mean_loss=0.0, linear=0)


@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_td_loss_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_TD_LOSS, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_TD_LOSS) == set(NEW_SYMBOLS)
    assert re.search(r"XQ_LOSS_SQUARED\s*=\s*0\s*,\s*XQ_LOSS_HUBER\s*=\s*1", text)
    assert (capi.LOSS_SQUARED, capi.LOSS_HUBER) == (0, 1)


def test_td_loss_on_a_null_handle_fails_loudly(capi):
    """No device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message; and
    DQN.set_td_loss refuses an unknown kind and a kappa that is not positive before it reaches the library."""
    k, x, a = C.c_int32(), C.c_double(), C.c_uint64()
    calls = [("xq_dqn_set_td_loss", (None, 1, 1.0)), ("xq_dqn_get_td_loss", (None, C.byref(k), C.byref(x))),
             ("xq_dqn_td_error_stats", (None, C.byref(a), C.byref(x), None, None, None))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name
    import cn_chess_ai_amd as xq
    d = xq.DQN.__new__(xq.DQN)
    d._h, d._own = None, False
    with pytest.raises(xq.XqError):
        d.set_td_loss("huber", 1.0)
    with pytest.raises(xq.XqError):
        d.td_error_stats()
    for bad in (0.0, -1.0, float("nan"), -math.inf):
        with pytest.raises(ValueError):
            d.set_td_loss("huber", bad)
    with pytest.raises(ValueError):
        d.set_td_loss("l1")


def build_huber_facade_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "huber_facade.cpp"), os.path.join(BUILD, "huber_facade"))


def test_huber_facade_probe_compiles():
    """xq::TdLoss, xq::DQN::setTdLoss / tdLoss / tdErrorStats and xq::ChessAI::setTdLoss with plain g++ (no HIP headers)"""
    assert os.path.exists(build_huber_facade_probe())
