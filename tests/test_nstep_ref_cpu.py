"""CPU checks of the n-step returns' reference (not gpu): tests/nstep_ref.py's per-row fp32 loop against an independent per-trajectory
walk in fp64, three wrong references told apart, every fixture of tests/test_nstep_gpu.py holding every class of row, and header,
ctypes table and library agreeing on the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nstep_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_replay_set_n_step", "xq_replay_get_n_step", "xq_replay_per_rebuild_hold", "xq_dqn_last_n_step",
               "xq_trainer_set_n_step")
GAMMA = 0.97
N_VALUES = (2, 3, 5, 8)


def reference(fx, slots, n, wrong=None):
    first, count = nr.readable(fx["cap"], fx["size"], fx["write_pos"])
    return nr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n, fx["stride"], GAMMA, first, count, wrong=wrong)


@pytest.mark.parametrize("name", list(nr.FIXTURES))
@pytest.mark.parametrize("n", N_VALUES)
def test_fp32_loop_agrees_with_the_fp64_trajectory_walk(name, n):
    fx = nr.named_fixture(name)
    slots = nr.all_slots(fx)
    ref = reference(fx, slots, n)
    walk = nr.trajectory_walk(fx, slots, n, fx["stride"], GAMMA)
    worst = 0.0
    for b, (R64, m, D, last, dead, mag) in enumerate(walk):
        assert (ref["steps"][b], bool(ref["done"][b]), ref["last_slot"][b], bool(ref["dead"][b])) == (m, D, last, dead), (b, slots[b])
        err = abs(float(ref["reward"][b]) - R64)
        assert err <= nr.reward_bound(n, mag) + 2.0 ** -149, (b, err, mag)
        worst = max(worst, err / mag if mag else 0.0)
    assert worst < 3 * n * 2.0 ** -24 * 1.01
    assert (ref["action"][ref["dead"]] == -1).all() and (ref["action"][~ref["dead"]] >= 0).all()


@pytest.mark.parametrize("name", list(nr.FIXTURES))
@pytest.mark.parametrize("wrong", ["ignore_done", "plus_one", "incomplete_live"])
def test_wrong_references_are_told_apart(name, wrong):
    """each negative control disagrees with the fp64 walk on (m, D, last slot, dead) of at least one row, at the fixture's own n"""
    fx = nr.named_fixture(name)
    n = nr.FIXTURES[name][3]
    slots = nr.all_slots(fx)
    bad = reference(fx, slots, n, wrong=wrong)
    walk = nr.trajectory_walk(fx, slots, n, fx["stride"], GAMMA)
    differ = sum((bad["steps"][b], bool(bad["done"][b]), bad["last_slot"][b], bool(bad["dead"][b])) != (m, D, last, dead)
                 for b, (_, m, D, last, dead, _) in enumerate(walk))
    assert differ > 0


@pytest.mark.parametrize("name", list(nr.FIXTURES))
def test_every_fixture_holds_every_class_of_row(name):
    """from the reference alone: the identity batch (the filled slots) of each fixture has a full chain, a chain that ends at done for
    every m in 1..n, an incomplete chain, an empty slot at k = 0 and one mid-chain"""
    fx = nr.named_fixture(name)
    cap, stride, pushes, n = nr.FIXTURES[name]
    ref = reference(fx, nr.filled_slots(fx), n)
    have = set(ref["cls"])
    assert set(nr.classes(n)) <= have, sorted(set(nr.classes(n)) - have)
    assert "cut" not in have
    if name.startswith("wrapped"):
        assert pushes > cap and fx["size"] == cap and fx["write_pos"] == pushes % cap
        assert fx["write_pos"] != 0 or name == "wrapped40"
    else:
        assert pushes < cap and fx["size"] == pushes
    assert cap % stride != 0 or name == "wrapped40"
    assert (n - 1) * stride < cap and (max(N_VALUES) - 1) * stride < cap


def test_discounts_round_once_per_factor():
    d = nr.discounts(0.99, 8)
    assert d[0] == np.float32(1.0) and d[1] == np.float32(0.99)
    for k in range(2, 9):
        assert d[k] == np.float32(np.float64(d[k - 1]) * np.float64(np.float32(0.99)))       # (a product of two floats is exact in fp64)
    assert d[3] != np.float32(0.99 ** 3) or d[8] != np.float32(0.99 ** 8)                     # not the rounded power


@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_n_step_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_N_STEP, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_N_STEP) == set(NEW_SYMBOLS)
    assert re.search(r"XQ_MAX_N_STEP\s*=\s*8", text) and capi.MAX_N_STEP == 8


def test_n_step_on_a_null_handle_fails_loudly(capi):
    """no device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message"""
    k = C.c_int32()
    calls = [("xq_replay_set_n_step", (None, 3, 4)), ("xq_replay_get_n_step", (None, C.byref(k), None)),
             ("xq_replay_per_rebuild_hold", (None, 0, 0, 0, 0)), ("xq_dqn_last_n_step", (None, 1, None, None, None, None, None, None)),
             ("xq_trainer_set_n_step", (None, 3))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name


def test_work_model_knows_the_new_brackets_only_when_asked():
    import cn_chess_ai_amd.workmodel as wm
    cfg = ((1260, 256, 256, 8100), 8192, 8192)
    base, same, on = wm.step_work(*cfg), wm.step_work(*cfg, n_step=1), wm.step_work(*cfg, n_step=3)
    assert base == same and "nstep_assemble" not in base and "per_writeback" not in base
    assert set(on) - set(base) == {"nstep_assemble"} and all(on[k] == base[k] for k in base)
    assert on["nstep_assemble"]["hbm_bytes"] == 8192 * (9 * 3 + 4 * 48 + 21) and on["nstep_assemble"]["bound"] == "hbm"
    per = wm.step_work(*cfg, n_step=3, prioritized=True)
    assert set(per) - set(wm.step_work(*cfg, prioritized=True)) == {"nstep_assemble", "per_writeback"}
    assert wm.rocprof_kernel("nstep_assemble", *cfg[:2]) == "nstep_assemble_kernel("
    assert wm.rocprof_kernel("per_writeback", *cfg[:2]) == "per_writeback_kernel("


def build_nstep_facade_probe():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "tests", "cpp", "nstep_facade.cpp"), os.path.join(BUILD, "nstep_facade"))


def test_nstep_facade_probe_compiles(capi):
    """xq::ReplayBuffer::setNStep / nStep, xq::ChessAI::setNStep / nStep and TrainStats::nStep with plain g++ (no HIP headers)"""
    assert os.path.exists(build_nstep_facade_probe())
