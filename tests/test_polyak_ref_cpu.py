"""CPU checks of the soft target update's reference and boundary (not gpu): tests/polyak_ref.py is torch.lerp in float64, equal online
and target bits are a fixed point, its one-step bound holds for an fp32 emulation of the device step and tells a wrong tau from the right
one, and header, ctypes table and library agree on the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polyak_ref as pr
from test_arena_cpu import gxx, BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_dqn_set_target_tau", "xq_dqn_get_target_tau", "xq_dqn_soft_update_target", "xq_trainer_set_target_tau")


def seeded_pairs(n, seed):
    """(t, p) fp32: magnitudes 1e-30 .. 1e4 of either sign, and slices with p == t, opposite signs, subnormals and |t| >> |p|"""
    rng = np.random.default_rng(seed)
    t = (10.0 ** rng.uniform(-30, 4, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    p = (10.0 ** rng.uniform(-30, 4, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    k = n // 10
    p[:k] = t[:k]                                                        # equal bits
    p[k:2 * k] = -t[k:2 * k]                                             # opposite signs, equal magnitude
    p[2 * k:3 * k] = (t[2 * k:3 * k] * np.float32(1 + 2.0 ** -20)).astype(np.float32)   # close: the difference cancels
    with np.errstate(under="ignore"):
        t[3 * k:4 * k] = (rng.uniform(-1, 1, size=k) * 1e-39).astype(np.float32)       # subnormal targets
        p[3 * k:4 * k] = (rng.uniform(-1, 1, size=k) * 1e-39).astype(np.float32)       # ... and online values
        p[4 * k:5 * k] = (rng.uniform(-1, 1, size=k) * 1e-41).astype(np.float32)
    t[5 * k:6 * k] = (rng.uniform(1e6, 1e9, size=k) * rng.choice([-1.0, 1.0], size=k)).astype(np.float32)   # |t| >> |p|
    p[5 * k:6 * k] = rng.uniform(-0.05, 0.05, size=k).astype(np.float32)
    p[6 * k:7 * k] = 0.0
    return t, p


@pytest.mark.parametrize("tau", [1e-3, 0.01, 0.3])
def test_polyak_ref_is_torch_lerp_in_float64(tau):
    import torch
    t, p = seeded_pairs(1 << 16, 3)
    t32 = pr.tau32(tau)
    ref = pr.step(t, p, t32)
    want = torch.lerp(torch.from_numpy(t.astype(np.float64)), torch.from_numpy(p.astype(np.float64)), float(t32)).numpy()
    scale = np.maximum(np.abs(want), np.maximum(np.abs(t), np.abs(p)).astype(np.float64) * float(t32))
    assert (np.abs(ref - want) <= 1e-15 * scale).all()
    assert np.abs(ref - t).max() > 0


def test_equal_bits_are_a_fixed_point():
    t, _ = seeded_pairs(1 << 16, 5)
    for tau in (1e-3, 0.01, 0.3, 0.999):
        t32 = pr.tau32(tau)
        assert np.array_equal(pr.step(t, t, t32), t.astype(np.float64))
        assert np.array_equal(pr.fp32_step(t, t, t32).view(np.uint32), t.view(np.uint32))
    assert (t != 0).all()
    # the one exception in bits, not in value: -0 meeting -0 gives d = +0 and fma(tau, +0, -0) = +0 (IEEE 754 round-to-nearest)
    z = np.array([0.0, -0.0], np.float32)
    got = pr.fp32_step(z, z, pr.tau32(0.3))
    assert np.array_equal(got, z) and np.array_equal(got.view(np.uint32), np.zeros(2, np.uint32))


@pytest.mark.parametrize("tau", [0.005, 0.01, 0.3])
def test_bound_holds_for_the_fp32_step_and_rejects_a_wrong_tau(tau):
    n = 1_000_000
    t, p = seeded_pairs(n, 11)
    t32 = pr.tau32(tau)
    ref, bound = pr.one_step_bound(t, p, t32)
    got = pr.fp32_step(t, p, t32).astype(np.float64)
    ratio = np.abs(got - ref) / bound
    print("polyak one-step err/bound, fp32 emulation", tau, float(ratio.max()))
    assert (ratio <= 1.0).all()
    assert ratio.max() > 0.25                                           # the bound is not slack by orders of magnitude
    k = n // 10
    assert np.array_equal(got[:k], t[:k].astype(np.float64))            # p == t
    # the element rule at tau = 1 does not reproduce p where |t| >> |p| (why tau = 1 is defined as the copy)
    one = pr.fp32_step(t[5 * k:6 * k], p[5 * k:6 * k], np.float32(1.0))
    assert (one != p[5 * k:6 * k]).mean() > 0.5
    # a tau one part in a thousand off, or a step that forgets the old target, is outside the bound on most elements that move
    # (where the step tau |p - t| is not small against |t| — there u |t| dominates the bound — and nothing is subnormal)
    moving = (np.abs(p.astype(np.float64) - t) > np.abs(t)) & (np.abs(p.astype(np.float64) - t) > 1e-30)
    assert moving.mean() > 0.2
    wrong = pr.fp32_step(t, p, np.float32(tau * 1.001)).astype(np.float64)
    assert (np.abs(wrong - ref)[moving] > bound[moving]).mean() > 0.9
    copied = p.astype(np.float64)
    assert (np.abs(copied - ref)[moving] > bound[moving]).mean() > 0.9


def test_budget_follows_a_trajectory_of_fp32_steps():
    rng = np.random.default_rng(2)
    n, t32 = 1 << 14, pr.tau32(0.01)
    t = rng.uniform(-0.05, 0.05, size=n).astype(np.float32)
    p = rng.uniform(-0.05, 0.05, size=n).astype(np.float32)
    B = pr.Budget(t)
    for _ in range(20):
        p = (p + rng.normal(0, 1e-3, size=n)).astype(np.float32)
        t1 = pr.fp32_step(t, p, t32)
        ref, bound = B.advance(t, p, t32)
        assert (np.abs(t1.astype(np.float64) - ref) <= bound).all()
        t = t1
    assert bound.max() < 20 * 2.0 ** -23 * 0.06


@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_target_tau_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_TARGET_TAU, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_TARGET_TAU) == set(NEW_SYMBOLS)
    assert "xq_trainer_config" in text and "tau" not in re.search(r"typedef struct \{[^}]*\} xq_trainer_config;", text, re.S).group(0)
    assert "updateTargetNetwork" in open(HEADER).read().split("xq_dqn_set_target_tau(")[0][-2500:]     # cites what it extends


def test_target_tau_on_a_null_handle_fails_loudly(capi):
    """No device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message; the Python
    methods refuse a tau outside [0, 1] or NaN before it reaches the library."""
    x = C.c_double()
    calls = [("xq_dqn_set_target_tau", (None, 0.01)), ("xq_dqn_get_target_tau", (None, C.byref(x))),
             ("xq_dqn_soft_update_target", (None, 0.5)), ("xq_trainer_set_target_tau", (None, 0.01))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name
    import cn_chess_ai_amd as xq
    d = xq.DQN.__new__(xq.DQN)
    d._h, d._own = None, False
    with pytest.raises(xq.XqError):
        d.set_target_tau(0.01)
    with pytest.raises(xq.XqError):
        d.target_tau()
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            d.set_target_tau(bad)
        with pytest.raises(ValueError):
            d.updateTargetNetwork(bad)
    t = xq.Trainer.__new__(xq.Trainer)
    t._h = None
    with pytest.raises(ValueError):
        t.set_target_tau(2.0)


def test_workmodel_prices_the_soft_update_only_when_asked():
    from cn_chess_ai_amd import workmodel as wm
    cfg = ((1260, 256, 256, 8100), 8192, 8192)
    touched = 1260 * 256 + 256 * 256 + 96 * 256 + 96 + 512
    for opt, name in (("sgd", "sgd_apply"), ("adam", "adam_apply")):
        base, soft = wm.step_work(*cfg, optimizer=opt), wm.step_work(*cfg, optimizer=opt, soft_target=True)
        assert set(base) == set(soft) and {k for k in base if base[k] != soft[k]} == {name}
        assert soft[name]["hbm_bytes"] == base[name]["hbm_bytes"] + 8 * touched        # the touched target read and written once


def build_soft_target_facade_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "soft_target_facade.cpp"), os.path.join(BUILD, "soft_target_facade"))


def test_soft_target_facade_probe_and_examples_compile():
    """xq::DQN::setTargetTau / targetTau / updateTargetNetwork(tau) / xq::ChessAI::setTargetTau with plain g++ (no HIP headers), and the
    examples against the new header"""
    assert os.path.exists(build_soft_target_facade_probe())
    for ex in ("train_selfplay", "arena"):
        assert os.path.exists(gxx(os.path.join(ROOT, "examples", ex + ".cpp"), os.path.join(BUILD, ex + "_soft_target")))
