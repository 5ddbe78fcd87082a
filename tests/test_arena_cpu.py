"""Arena (DESIGN.md §4 "Arena") without a device: the host summary, the C++ facade and examples/arena.cpp compile with plain g++."""
import os
import subprocess

import numpy as np

from cn_chess_ai_amd import arena as xa
from cn_chess_ai_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")


def gxx(src, out):
    os.makedirs(BUILD, exist_ok=True)
    pkg = os.path.join(ROOT, "cn_chess_ai_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", out, f"-I{os.path.join(ROOT, 'include')}", f"-L{pkg}",
                           "-lxqhip", f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"])
    return out


def build_example():
    return gxx(os.path.join(ROOT, "examples", "arena.cpp"), os.path.join(BUILD, "arena"))


def build_facade_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "arena_facade.cpp"), os.path.join(BUILD, "arena_facade"))


def test_example_and_facade_compile_with_plain_gxx():
    assert os.path.exists(build_example())
    assert os.path.exists(build_facade_probe())


def records(results, causes, pairs):
    r = np.zeros(2 * pairs, dtype=xa.GAME_DTYPE)
    r["a_result"], r["cause"] = results, causes
    r["a_is_red"][:pairs] = 1
    return r


def test_summary_counts_and_pair_interval():
    C = _capi.ARENA_GENERAL_CAPTURED
    # pairs: (win, loss) (win, win) (draw, draw) (loss, loss) + one pair decided inside the opening
    res = [1, 1, 0, -1, 0, -1, 1, 0, -1, 0]
    cause = [C, C, _capi.ARENA_MOVE_CAP, C, _capi.ARENA_OPENING] + [C, C, _capi.ARENA_MOVE_CAP, C, _capi.ARENA_OPENING]
    s = xa.summarize(records(res, cause, 5), 5)
    assert (s["wins"], s["draws"], s["losses"], s["scored_games"], s["scored_pairs"]) == (3, 2, 3, 8, 4)
    assert s["causes"]["opening"] == 2 and s["causes"]["move_cap"] == 2 and s["causes"]["general_captured"] == 6
    assert s["score"] == 0.5 and s["elo"] == 0.0
    pair = np.array([0.5, 1.0, 0.5, 0.0])
    half = 1.96 * np.sqrt(pair.var(ddof=1) / 4)
    assert np.isclose(s["ci95"][0], 0.5 - half) and np.isclose(s["ci95"][1], 0.5 + half)


def test_summary_clamps_elo_and_skips_live_games():
    C = _capi.ARENA_GENERAL_CAPTURED
    s = xa.summarize(records([1, 1, 1, 1], [C, C, C, C], 2), 2)
    assert s["score"] == 1.0 and np.isfinite(s["elo"]) and s["elo"] > 0
    s = xa.summarize(records([0, 0], [_capi.ARENA_LIVE, _capi.ARENA_LIVE], 1), 1)
    assert s["scored_games"] == 0 and np.isnan(s["score"]) and s["causes"]["live"] == 2
