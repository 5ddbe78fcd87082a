"""CPU checks of the gradient clipping's reference and boundary (not gpu): tests/clip_ref.py is torch.nn.utils.clip_grad_norm_ in front
of torch.optim.SGD / Adam, its one-step bounds tell a wrong coefficient from the right one, and header, ctypes table and library agree
on the new entry points."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import adam_ref as ar
import clip_ref as cr
from test_arena_cpu import gxx, BUILD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_dqn_set_grad_clip", "xq_dqn_get_grad_clip", "xq_dqn_grad_clip_stats")
REF_NET = (1260, 128, 8100)


def segment_lengths(sizes):
    lay = ar.layout(sizes)
    offs = sorted([lay["w0"], *lay["wh"].values(), lay["wout"], lay["bout"], lay["bh"], lay["n"]])
    return [b - a for a, b in zip(offs[:-1], offs[1:])]


def gradients(rng, n, scale):
    g = scale * 10.0 ** rng.uniform(-6, 0, size=n) * rng.choice([-1.0, 1.0], size=n)
    g[rng.random(n) < 0.2] = 0.0
    return g


@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_clip_ref_is_torch_clip_grad_norm_then_the_optimizer(opt):
    import torch
    rng = np.random.default_rng(7)
    lens = segment_lengths(REF_NET)
    n, lr, gs, max_norm = sum(lens), 1e-2, 1.0 / 64, 0.5
    assert lens == [1260 * 128, 96 * 128, 96, 128]
    p0 = rng.uniform(-0.05, 0.05, size=n)
    cuts = np.cumsum(lens)[:-1]
    tps = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in np.split(p0, cuts)]
    topt = (torch.optim.SGD(tps, lr=lr) if opt == "sgd" else
            torch.optim.Adam(tps, lr=lr, betas=(ar.BETA1, ar.BETA2), eps=ar.EPS, weight_decay=0.0, amsgrad=False, foreach=False))
    p, m, v = p0.copy(), np.zeros(n), np.zeros(n)
    coefs = []
    for t, scale in enumerate([1e3, 1e-3, 30.0, 1e-1, 1e4, 3.0], start=1):      # norms far above, far below and near max_norm
        g = gradients(rng, n, scale)
        for tp, x in zip(tps, np.split(gs * g, cuts)):
            tp.grad = torch.tensor(x, dtype=torch.float64)
        total = float(torch.nn.utils.clip_grad_norm_(tps, max_norm, foreach=False))
        topt.step()
        nrm = cr.norm(g, gs)
        c = cr.coef(g, max_norm, gs)
        coefs.append(c)
        assert abs(nrm - total) <= 1e-13 * total
        if opt == "sgd":
            p = cr.sgd_step(p, g, lr, gs, c)
        else:
            p, m, v = cr.adam_step(p, m, v, g, t, lr, gs, c)
        want = np.concatenate([tp.detach().numpy() for tp in tps])
        assert np.allclose(p, want, rtol=1e-12, atol=1e-12 * lr), t
        if opt == "adam":
            want_v = np.concatenate([topt.state[tp]["exp_avg_sq"].numpy() for tp in tps])
            assert np.allclose(v, want_v, rtol=1e-11, atol=0)
    assert min(coefs) < 1e-2 and coefs.count(1.0) >= 2 and any(0.05 < c < 1.0 for c in coefs), coefs
    assert cr.coef(np.zeros(8), 1.0) == 1.0 and cr.coef(g, math.inf, gs) == 1.0 and cr.coef(g, 0.25 * nrm, gs) < 0.25


def fp32_sgd(p, g, lr, gs, c):
    """the definition in fp32, one rounding per operation: what a correct kernel may do"""
    f = np.float32
    alpha = f(f(lr * gs) * f(c))
    return np.asarray(p, f) - alpha * np.asarray(g, f)


def test_sgd_bound_rejects_a_wrong_coefficient():
    """The fp32 step with the global coefficient lies inside the bound; one clipped per segment, and one without the 1e-6, leave it."""
    rng = np.random.default_rng(13)
    lens = segment_lengths(REF_NET)
    n, lr, gs = sum(lens), 1.0, 1.0
    cuts = np.cumsum(lens)[:-1]
    p0 = np.zeros(n, np.float32)
    g = gradients(rng, n, 1e-4).astype(np.float32)
    nrm = cr.norm(g, gs)
    assert 1e-3 < nrm < 1e-1
    max_norm = 0.1 * nrm
    c = cr.coef(g, max_norm, gs)
    ref, bound = cr.sgd_one_step_bound(p0, g, lr, gs, c)
    ok = fp32_sgd(p0, g, lr, gs, c).astype(np.float64)
    assert (np.abs(ok - ref) <= bound).all() and (np.abs(ok - ref) / bound).max() > 0.01
    per_segment = np.concatenate([cr.coef(x, max_norm, gs) * np.ones(x.size) for x in np.split(g, cuts)])
    wrong = fp32_sgd(p0, g, lr, gs, per_segment.astype(np.float32)).astype(np.float64)
    assert (np.abs(wrong - ref) > bound).sum() > n // 100
    c_no_eps = min(1.0, max_norm / nrm)
    assert abs(c_no_eps - c) / c > 1e-5
    wrong = fp32_sgd(p0, g, lr, gs, c_no_eps).astype(np.float64)
    assert (np.abs(wrong - ref) > bound).sum() > n // 100


def test_adam_bound_holds_for_the_fp32_step_and_rejects_a_wrong_coefficient():
    from test_adam_ref_cpu import fp32_step
    rng = np.random.default_rng(17)
    n, lr, gs = 1 << 14, 1e-3, 1.0 / 3.0
    p = rng.uniform(-0.05, 0.05, size=n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(1, 6):
        g = (10.0 ** rng.uniform(-12, 4, size=n) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
        g[rng.random(n) < 0.2] = 0.0
        c = cr.coef(g, 0.3 * cr.norm(g, gs), gs)
        (rp, rm, rv), (bp, bm, bv) = cr.adam_one_step_bound(p, m, v, g, t, lr, gs, c)
        scale = np.float32(np.float32(gs) * np.float32(c))
        with np.errstate(under="ignore"):
            p1, m1, v1 = fp32_step(p, m, v, g, t, lr, scale)
        for x, r, b in ((p1, rp, bp), (m1, rm, bm), (v1, rv, bv)):
            assert (np.abs(x.astype(np.float64) - r) <= b).all(), t
        with np.errstate(under="ignore"):
            _, wm, _ = fp32_step(p, m, v, g, t, lr, np.float32(gs))           # not clipped at all
        assert (np.abs(wm.astype(np.float64) - rm) > bm).sum() > n // 2
        p, m, v = p1, m1, v1


@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_grad_clip_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_GRAD_CLIP, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_GRAD_CLIP) == set(NEW_SYMBOLS)


def test_grad_clip_on_a_null_handle_fails_loudly(capi):
    """No device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message; and
    DQN.set_grad_clip refuses a negative or NaN max_norm before it reaches the library."""
    x, a = C.c_double(), C.c_uint64()
    calls = [("xq_dqn_set_grad_clip", (None, 1.0)), ("xq_dqn_get_grad_clip", (None, C.byref(x))),
             ("xq_dqn_grad_clip_stats", (None, C.byref(x), None, C.byref(a), None))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name
    import cn_chess_ai_amd as xq
    d = xq.DQN.__new__(xq.DQN)
    d._h, d._own = None, False
    with pytest.raises(xq.XqError):
        d.set_grad_clip(1.0)
    with pytest.raises(xq.XqError):
        d.grad_clip_stats()
    for bad in (-1.0, -0.5, float("nan"), -math.inf):
        with pytest.raises(ValueError):
            d.set_grad_clip(bad)


def test_workmodel_prices_grad_norm_only_when_asked():
    from cn_chess_ai_amd import workmodel as wm
    cfg = ((1260, 256, 256, 8100), 8192, 8192)
    base, clip = wm.step_work(*cfg), wm.step_work(*cfg, grad_clip=True)
    assert "grad_norm" not in base and set(clip) - set(base) == {"grad_norm"}
    touched = 1260 * 256 + 256 * 256 + 96 * 256 + 96 + 512
    slabs = base["sgd_apply"]["hbm_bytes"] / 4 - 2 * touched
    assert clip["grad_norm"]["hbm_bytes"] == 4 * (slabs + touched) and clip["grad_norm"]["bound"] == "hbm"
    assert clip["sgd_apply"]["hbm_bytes"] == 4 * 3 * touched                   # the buffer, and the parameters read and written
    assert {k for k in base if base[k] != clip[k]} == {"sgd_apply"}
    adam = wm.step_work(*cfg, grad_clip=True, optimizer="adam")
    assert adam["adam_apply"]["hbm_bytes"] == 4 * 3 * touched + 16 * touched and "sgd_apply" not in adam


def build_clip_facade_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "clip_facade.cpp"), os.path.join(BUILD, "clip_facade"))


def test_clip_facade_probe_and_example_compile():
    """xq::DQN::setGradClip / gradClip / gradClipStats / xq::ChessAI::setGradClip with plain g++ (no HIP headers), and the example that
    takes clip=<max_norm>"""
    assert os.path.exists(build_clip_facade_probe())
    assert os.path.exists(gxx(os.path.join(ROOT, "examples", "train_selfplay.cpp"), os.path.join(BUILD, "train_selfplay_clip")))
    assert "clip=" in open(os.path.join(ROOT, "examples", "train_selfplay.cpp")).read()
