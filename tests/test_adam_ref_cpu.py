"""CPU checks of the Adam optimizer's reference and boundary (not gpu): tests/adam_ref.py is torch.optim.Adam, its one-step bound
tells a wrong formula from a right one, and header, ctypes table and library agree on the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adam_ref as ar
from test_arena_cpu import gxx, BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_dqn_set_optimizer", "xq_dqn_get_optimizer", "xq_dqn_reset_optimizer", "xq_dqn_get_optimizer_state",
               "xq_dqn_set_optimizer_state")


def gradients(rng, steps, n):
    """per step: magnitudes 1e-12 .. 1e4 (log-uniform), random signs that flip from step to step, a fifth of the entries exactly 0"""
    out = []
    for _ in range(steps):
        g = 10.0 ** rng.uniform(-12, 4, size=n) * rng.choice([-1.0, 1.0], size=n)
        g[rng.random(n) < 0.2] = 0.0
        out.append(g)
    out[1][:n // 4] = -out[0][:n // 4]              # exact sign flips of the same magnitude
    out[2][:8] = 0.0; out[3][:8] = 0.0             # entries that stay zero for a while after having moved
    return out


@pytest.mark.parametrize("lr,b1,b2,eps,gs", [(1e-3, 0.9, 0.999, 1e-8, 1.0), (3e-2, 0.5, 0.99, 1e-5, 1.0 / 8192)])
def test_adam_ref_is_torch_adam(lr, b1, b2, eps, gs):
    import torch
    rng = np.random.default_rng(5)
    n, steps = 4096, 50
    p0 = rng.uniform(-0.05, 0.05, size=n)
    gs_list = gradients(rng, steps, n)
    tp = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=lr, betas=(b1, b2), eps=eps, weight_decay=0.0, amsgrad=False, foreach=False)
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    sm = np.zeros(n)                                 # the size of the terms m is made of: where the signs flip m itself cancels
    for t, g in enumerate(gs_list, start=1):
        sm = b1 * sm + (1.0 - b1) * np.abs(gs * g)
        tp.grad = torch.tensor(gs * g, dtype=torch.float64)
        opt.step()
        p, m, v = ar.step(p, m, v, g, t, lr, gs, b1, b2, eps)
        st = opt.state[tp]
        want_p, want_m, want_v = tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
        assert np.abs(p - want_p).max() <= 1e-12 * np.abs(want_p).max()
        assert np.allclose(p, want_p, rtol=1e-12, atol=1e-12 * lr)
        assert (np.abs(m - want_m) <= 1e-12 * sm).all() and np.allclose(v, want_v, rtol=1e-12, atol=0)
    assert int(opt.state[tp]["step"]) == steps and np.abs(p - p0).max() > 10 * lr


def fp32_step(p, m, v, g, t, lr, gs, b1=ar.BETA1, b2=ar.BETA2, eps=ar.EPS):
    """the definition evaluated in fp32 one operation at a time (numpy rounds every operation once): what a correct kernel may do"""
    f = np.float32
    p, m, v, g = (np.asarray(x, dtype=f) for x in (p, m, v, g))
    gp = f(gs) * g
    m = f(b1) * m + f(1.0 - b1) * gp
    v = f(b2) * v + (f(1.0 - b2) * gp) * gp
    a, rbc2 = f(lr / (1.0 - b1 ** t)), f(1.0 / np.sqrt(1.0 - b2 ** t))
    den = np.sqrt(v) * rbc2 + f(eps)
    return p - a * (m / den), m, v


def test_one_step_bound_separates_right_from_wrong():
    """A step computed in fp32 as defined stays inside the one-step bound from any state; the same step without the bias correction, or
    with eps inside the square root, leaves it by more than 100 x on the same inputs."""
    rng = np.random.default_rng(11)
    n, lr, gs = 1 << 14, 1e-3, 1.0 / 3.0
    p = rng.uniform(-0.05, 0.05, size=n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for t in range(1, 21):
        g = (10.0 ** rng.uniform(-12, 4, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
        g[rng.random(n) < 0.2] = 0.0
        g[:64] = (rng.uniform(-1, 1, size=64) * 1e-38).astype(np.float32)           # subnormal-scale entries
        (rp, rm, rv), (bp, bm, bv) = ar.one_step_bound(p, m, v, g, t, lr, gs)
        with np.errstate(under="ignore"):
            p1, m1, v1 = fp32_step(p, m, v, g, t, lr, gs)
        ratios = [float((np.abs(x.astype(np.float64) - r) / b).max()) for x, r, b in ((p1, rp, bp), (m1, rm, bm), (v1, rv, bv))]
        assert max(ratios) <= 1.0, (t, ratios)
        worst = max(worst, max(ratios))
        for wrong in (dict(bias_correction=False), dict(eps_inside_sqrt=True)):
            wp, _, _ = ar.step(p, m, v, g, t, lr, gs, **wrong)
            assert (np.abs(wp - rp) / bp).max() > 100.0, (t, wrong)
        p, m, v = p1, m1, v1
    assert worst > 0.01                              # the bound is not vacuous either


def test_gradient_error_bound_covers_a_perturbed_gradient():
    rng = np.random.default_rng(3)
    n, lr = 1 << 14, 1e-3
    for t in (1, 2, 50):
        m0 = rng.normal(size=n) * 10.0 ** rng.uniform(-6, 0, size=n) * (t > 1)
        v0 = (np.abs(m0) * rng.uniform(1.0, 3.0, size=n)) ** 2
        gp = rng.normal(size=n) * 10.0 ** rng.uniform(-8, 1, size=n)
        E = np.abs(gp) * 10.0 ** rng.uniform(-7, 0.5, size=n)
        p0 = np.zeros(n)
        ref, _, _ = ar.step(p0, m0, v0, gp, t, lr)
        bound = ar.gradient_error_bound(m0, v0, gp, E, t, lr)
        for s in (-1.0, 1.0, 0.37):
            got, _, _ = ar.step(p0, m0, v0, gp + s * E, t, lr)
            # (+ the resolution of the fp64 evaluation itself: some E are below an ulp64 of the step)
            assert (np.abs(got - ref) <= bound * (1 + 1e-9) + 8 * np.finfo(np.float64).eps * np.abs(ref)).all()


def test_layout_round_trip():
    for sizes in ((1260, 128, 8100), (1260, 256, 256, 8100), (1260, 127, 129, 8100)):
        lay = ar.layout(sizes)
        buf = np.arange(1, lay["n"] + 1, dtype=np.float64)
        w, b = ar.to_reference(sizes, buf)
        cw, cb = ar.covered(sizes)
        assert cw.sum() + cb.sum() == lay["n"] and sorted(np.concatenate([w[cw], b[cb]])) == list(buf)
        L = sizes
        assert w[1] == buf[L[1]] and w[L[0]] == buf[1]                   # W0 is kept transposed on the device
        wo = sum(L[i] * L[i + 1] for i in range(len(L) - 2))
        assert not cw[wo + 96 * L[-2]:].any() and cw[:wo + 96 * L[-2]].all()
        assert not cb[sum(L[1:-1]) + 96:].any()


@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_optimizer_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert re.search(r"enum\s*\{\s*XQ_OPT_SGD\s*=\s*0\s*,\s*XQ_OPT_ADAM\s*=\s*1\s*\}", text)
    assert (capi.OPT_SGD, capi.OPT_ADAM) == (0, 1)
    assert set(capi.LAZY) == set(NEW_SYMBOLS)        # everything else must be there at load time


def test_set_optimizer_on_a_null_handle_fails_loudly(capi):
    """No device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message."""
    k, t = C.c_int32(), C.c_uint64()
    f = (C.c_float * 4)()
    calls = [("xq_dqn_set_optimizer", (None, capi.OPT_ADAM, 0.0, 0.0, 0.0)), ("xq_dqn_reset_optimizer", (None,)),
             ("xq_dqn_get_optimizer", (None, C.byref(k), None, None, None, C.byref(t))),
             ("xq_dqn_get_optimizer_state", (None, f, f, C.byref(t))), ("xq_dqn_set_optimizer_state", (None, f, f, 0))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name
    import cn_chess_ai_amd as xq
    d = xq.DQN.__new__(xq.DQN)
    d._h, d._own = None, False
    with pytest.raises(xq.XqError):
        d.set_optimizer("adam")
    with pytest.raises(ValueError):
        d.set_optimizer("rmsprop")


def build_adam_facade_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "adam_facade.cpp"), os.path.join(BUILD, "adam_facade"))


def test_adam_facade_probe_and_example_compile():
    """xq::Optimizer / xq::DQN::setOptimizer / xq::ChessAI::setOptimizer with plain g++ (no HIP headers), and the example that takes `adam`"""
    assert os.path.exists(build_adam_facade_probe())
    assert os.path.exists(gxx(os.path.join(ROOT, "examples", "train_selfplay.cpp"), os.path.join(BUILD, "train_selfplay_adam")))
