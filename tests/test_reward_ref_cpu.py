"""CPU checks of the reward rule (not gpu): tests/reward_ref.py against the oracle's own capture bookkeeping along self-play and versus
replays, the telescoping sum, the formula against fp64, the clamp, the argument rules, a fused formula told apart (negative control), and
header, ctypes table, library and facade agreeing on the new entry points."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import reward_ref as rr
import versus_ref as vr
import xqoracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "xq_capi.h")
NEW_SYMBOLS = ("xq_env_set_reward", "xq_env_get_reward", "xq_trainer_set_reward")
SEED, FIRST = 0x5EED, 1000
# the parameters of the GPU tests: at scale 1/1000, cost 0.003 a fused multiply-add rounds delta = 10, 40 and 1000 differently
GPU_PARAMS = (1.0 / 1000, 0.003, np.inf)


@pytest.fixture(scope="module")
def selfplay_run():
    """32 games x 120 plies of uniform-random self-play on the oracle (the GPU test's run), every ply's record"""
    sp = rr.SelfPlay(32, SEED, FIRST)
    return sp, [sp.step() for _ in range(120)]


@pytest.fixture(scope="module")
def versus_random():
    return rr.versus_run(32, 80, SEED, FIRST, vr.Opponent(vr.RANDOM), GPU_PARAMS)


# ---- delta from the boards is what was captured --------------------------------------------------------------------------------------
def test_selfplay_delta_from_boards_is_the_captured_value(selfplay_run):
    sp, plies = selfplay_run
    seen = 0
    for rows in plies:
        for s, to, value, mover, s2, _, _ in rows:
            if to < 0:
                assert np.array_equal(s, s2)
                continue
            assert rr.mover_of(s2, to) == mover
            assert rr.delta(s, s2, mover) == value >= 0 and rr.delta(s, s2, 1 - mover) == -value
            seen += value > 0
    # the census the GPU test leans on: all seven victim types, generals included
    assert {rr.TYPES[t - 1]: c for t, c in sp.victims.items()} == dict(soldier=114, horse=48, cannon=48, chariot=25, advisor=24,
                                                                       elephant=23, general=14)
    assert seen == sum(sp.victims.values())


def test_selfplay_boards_of_the_replay_are_the_oracles(selfplay_run):
    """s' of a ply is s of the game's next ply unless the game ended there (then the next s is the start position)"""
    _, plies = selfplay_run
    start = xo.new_board().squares()
    for a, b in zip(plies, plies[1:]):
        for (_, to, _, _, s2, _, done), (s_next, *_r) in zip(a, b):
            assert np.array_equal(s_next, s2) or np.array_equal(s_next, start)


def test_sum_of_deltas_telescopes_to_the_final_balance(selfplay_run):
    _, plies = selfplay_run
    start = xo.new_board().squares()
    for g in range(32):
        total, games = 0, 0
        for rows in plies:
            s, to, value, mover, s2, _, _ = rows[g]
            if np.array_equal(s, start):
                total = 0                                             # a new game
                games += 1
            total += rr.delta(s, s2, 0)                               # Red's view of every ply: + its own gains, - Black's
            assert rr.delta(s, s2, 0) == (value if mover == 0 else -value)
            assert total == rr.balance(s2, 0) == -rr.balance(s2, 1)
        assert games >= 1


def test_versus_delta_is_the_learners_gain_minus_the_replys(versus_random):
    slots, deltas, results = versus_random
    assert all(d == took - lost and took + lost == scored for _, d, took, lost, scored in deltas)
    ds = [d for _, d, _, _, _ in deltas]
    assert 1000 in ds and -1000 in ds
    both = [(d, took, lost) for _, d, took, lost, _ in deltas if took > 0 and lost > 0]
    assert len(both) >= 1
    res = [r for _, r in results]
    assert res.count(1) > 0 and res.count(-1) > 0
    # every written slot carries the formula of the delta of its own two boards
    n_empty = 0
    for collect in slots:
        for g, (s, to, r, done, s2) in enumerate(collect):
            side = (FIRST + g) & 1
            if to < 0 and r == 0 and isinstance(r, int):
                n_empty += 1                                          # the opponent's pre-move ended the game: reward 0 as it was
                continue
            assert np.float32(r).view(np.uint32) == rr.ring_reward(s, to, s2, GPU_PARAMS, side).view(np.uint32)


# ---- the formula ---------------------------------------------------------------------------------------------------------------------
PARAM_SETS = [(1e-3, 0.0, 1.0), (1e-3, 0.0, np.inf), GPU_PARAMS, (1.0 / 1000, 0.003, 0.5), (0.37, 1.25, 100.0), (3.0, 0.0, np.inf)]
DELTAS = sorted(set(range(-1000, 1001, 7)) | {-1000, -90, -45, -40, -25, -20, -10, 0, 10, 20, 40, 45, 80, 90, 1000})


@pytest.mark.parametrize("params", PARAM_SETS)
def test_formula_is_within_one_ulp_of_fp64_and_exact_without_a_cost(params):
    """Two roundings, each at most half an ulp of its own result: the product's at the product's magnitude, the difference's at the
    result's — together at most one ulp at the larger of the two magnitudes (the clamp only moves the value towards the fp64 one)."""
    for d in DELTAS:
        got, want = rr.formula(d, *params), rr.formula_fp64(d, *params)
        mag = max(abs(d * float(np.float32(params[0]))), abs(want))
        assert abs(float(got) - want) <= float(np.spacing(np.float32(mag))), (d, params)
        if np.float32(params[1]) == 0:
            assert got.view(np.uint32) == np.float32(want).view(np.uint32), (d, params)      # one rounding: the correctly rounded value


@pytest.mark.parametrize("params", PARAM_SETS)
def test_clamp_holds(params):
    b32 = np.float32(params[2])
    vals = np.array([rr.formula(d, *params) for d in DELTAS])
    assert (np.abs(vals) <= b32).all() and vals.dtype == np.float32
    assert (np.diff(vals) >= 0).all()                                 # monotone in delta
    if np.isfinite(b32) and 1000 * params[0] - params[1] > params[2]:
        assert vals[-1] == b32 and vals[0] == -b32                    # the general is clamped on both sides
    if not np.isfinite(b32):
        assert vals[-1] == np.float32(np.float32(np.float32(1000) * np.float32(params[0])) - np.float32(params[1]))


def test_default_parameters_bound_the_reward_to_the_tanh_range():
    assert rr.formula(1000, *rr.DEFAULTS) == np.float32(1.0) and rr.formula(-1000, *rr.DEFAULTS) == np.float32(-1.0)
    assert rr.formula(90, *rr.DEFAULTS) == np.float32(np.float32(90) * np.float32(1e-3)) and rr.formula(0, *rr.DEFAULTS) == 0


def test_fused_formula_differs_at_the_gpu_tests_parameters():
    """NEGATIVE CONTROL: a kernel that contracts the product into the difference is told apart by the victims that occur"""
    for d in (10, 40, 1000):
        assert rr.formula(d, *GPU_PARAMS).view(np.uint32) != rr.formula_fused(d, *GPU_PARAMS).view(np.uint32), d
    assert all(rr.formula(d, 1e-3, 0.0, 1.0) == rr.formula_fused(d, 1e-3, 0.0, 1.0) for d in DELTAS)      # nothing to fuse without a cost


def test_argument_rules():
    inf, nan = np.inf, np.nan
    good = [(0, 1e-3, 0.0, 1.0), (1, 1e-3, 0.0, 1.0), (1, 1e-3, 0.0, inf), (1, 5.0, 2.0, 1e-6), (1, 1e-30, 0.0, 1.0)]
    bad = [(2, 1e-3, 0.0, 1.0), (-1, 1e-3, 0.0, 1.0), (1, 0.0, 0.0, 1.0), (1, -1e-3, 0.0, 1.0), (1, inf, 0.0, 1.0), (1, nan, 0.0, 1.0),
           (1, 1e-3, -0.1, 1.0), (1, 1e-3, inf, 1.0), (1, 1e-3, nan, 1.0), (1, 1e-3, 0.0, 0.0), (1, 1e-3, 0.0, -1.0), (1, 1e-3, 0.0, nan),
           (1, 1e-60, 0.0, 1.0), (1, 1e60, 0.0, 1.0), (0, nan, 0.0, 1.0)]          # (a scale that is 0 or inf as fp32 is refused too)
    assert all(rr.args_ok(*a) for a in good) and not any(rr.args_ok(*a) for a in bad)


# ---- header, ctypes table, library, facade ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def capi():
    lib = os.path.join(ROOT, "cn_chess_ai_amd", "libxqhip.so")
    if not os.path.exists(lib):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "cn_chess_ai_amd", "csrc"), "all"])
    from cn_chess_ai_amd import _capi
    _capi.load()
    return _capi


def test_reward_symbols_are_declared_exported_and_bound(capi):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(xq_[a-z0-9_]+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH]).decode()
    exported = set(re.findall(r" T (xq_[a-z0-9_]+)", out))
    lib = capi.load()
    for n in NEW_SYMBOLS:
        assert n in declared and n in exported and n in capi.PROTOTYPES and n in capi.LAZY_REWARD, n
        assert getattr(lib, n).argtypes == capi.PROTOTYPES[n]
    assert set(capi.LAZY_REWARD) == set(NEW_SYMBOLS)
    assert (capi.REWARD_EVALUATE, capi.REWARD_DELTA) == (rr.EVALUATE, rr.DELTA) == (0, 1)
    assert re.search(r"XQ_REWARD_EVALUATE\s*=\s*0\s*,\s*XQ_REWARD_DELTA\s*=\s*1", text)


def test_reward_on_a_null_handle_fails_loudly(capi):
    """no device is needed to be refused: a NULL handle is XQ_ERR_INVALID_ARGUMENT from every new entry point, with a message"""
    k, s, c, b = C.c_int32(), C.c_double(), C.c_double(), C.c_double()
    calls = [("xq_env_set_reward", (None, 1, 1e-3, 0.0, 1.0)), ("xq_env_get_reward", (None, C.byref(k), C.byref(s), C.byref(c), C.byref(b))),
             ("xq_trainer_set_reward", (None, 1, 1e-3, 0.0, 1.0))]
    for name, args in calls:
        with pytest.raises(capi.XqError) as e:
            capi.call(name, *args)
        assert e.value.code == 1 and "null" in str(e.value).lower(), name


def test_python_wrapper_names_the_kinds():
    from cn_chess_ai_amd import vecenv
    assert vecenv.reward_kind("evaluate") == 0 and vecenv.reward_kind("delta") == 1 and vecenv.reward_kind(1) == 1
    with pytest.raises(ValueError):
        vecenv.reward_kind("material")


def build_reward_facade_probe():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "tests", "cpp", "reward_facade.cpp"), os.path.join(BUILD, "reward_facade"))


def build_train_selfplay():
    from test_arena_cpu import gxx, BUILD
    return gxx(os.path.join(ROOT, "examples", "train_selfplay.cpp"), os.path.join(BUILD, "train_selfplay_reward"))


def test_train_selfplay_parses_the_reward_argument(capi):
    """reward=evaluate | delta[:scale[:cost[:bound]]]; a malformed one ends the program with status 2 before anything touches a device"""
    exe = build_train_selfplay()
    for bad in ("reward=", "reward=material", "reward=deltas", "reward=delta:", "reward=delta:x", "reward=delta:1e-3:0:1:2",
                "reward=delta:1e-3,0"):
        r = subprocess.run([exe, "1", os.devnull, "64", bad], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "reward=" in r.stderr, (bad, r.returncode, r.stderr)


def test_reward_facade_probe_compiles(capi):
    """xq::Reward, xq::VecEnv::setReward / reward, xq::ChessAI::setReward / reward and TrainStats::reward with plain g++ (no HIP headers)"""
    assert os.path.exists(build_reward_facade_probe())
