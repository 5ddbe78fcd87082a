"""The zero-sum target's entry points (not gpu): include/xq_capi.h, the ctypes table, the library's exports and the Python and C++
surfaces agree on them; a NULL handle is refused with a message; the facade probe and the example compile with plain g++."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_dqn_set_zero_sum", "xq_dqn_get_zero_sum", "xq_trainer_set_zero_sum")


@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_zero_sum_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_ZERO_SUM, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_ZERO_SUM) == set(NEW_SYMBOLS)
    assert not set(capi.LAZY_ZERO_SUM) & (set(capi.LAZY_LEGAL) | set(capi.LAZY_REWARD) | set(capi.LAZY_COLOUR_SWAP))


def test_prototypes_match_the_headers_parameter_lists(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    want = {"xq_dqn_set_zero_sum": ("xq_dqn* d, int on", [C.c_void_p, C.c_int32]),
            "xq_dqn_get_zero_sum": ("const xq_dqn* d, int* on", [C.c_void_p, C.POINTER(C.c_int32)]),
            "xq_trainer_set_zero_sum": ("xq_trainer* t, int on", [C.c_void_p, C.c_int32])}
    for name, (params, argtypes) in want.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m and " ".join(m.group(1).split()) == params, name
        assert capi.PROTOTYPES[name] == argtypes, name


def test_zero_sum_on_a_null_handle_fails_loudly(capi):
    """no device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message"""
    v = C.c_int32()
    for name, args in (("xq_dqn_set_zero_sum", (None, 1)), ("xq_dqn_get_zero_sum", (None, C.byref(v))),
                       ("xq_trainer_set_zero_sum", (None, 1))):
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name


def test_python_surface_has_the_setters():
    from cn_chess_ai_amd import dqn
    for cls, names in ((dqn.DQN, ("set_zero_sum", "zero_sum")), (dqn.Trainer, ("set_zero_sum",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def build_zero_sum_facade_probe():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "tests", "cpp", "zero_sum_facade.cpp"), os.path.join(BUILD, "zero_sum_facade"))


def build_example():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "examples", "train_selfplay.cpp"), os.path.join(BUILD, "train_selfplay_zero_sum"))


def test_zero_sum_facade_probe_and_example_compile(capi):
    """xq::DQN::setZeroSum / zeroSum, xq::ChessAI::setZeroSum / zeroSum and TrainStats::zero_sum with plain g++ (no HIP headers)"""
    assert os.path.exists(build_zero_sum_facade_probe())
    exe = build_example()
    out = subprocess.run([exe, "1", "m.bin", "1", "target=some"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "target=" in out.stderr
