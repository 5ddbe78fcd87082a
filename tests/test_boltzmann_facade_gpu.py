"""The exploration policy through the C++ facade and the examples: tests/cpp/policy_facade.cpp — xq::ChessAI::setPolicy / setEpsilon round
trips and refusals, the throws of the single-board paths, TrainStats::policy / epsilon / exploredPlies of batched runs,
xq::Arena::setTemperature — and examples/train_selfplay ... policy=boltzmann:T eps=E, examples/arena --temp-a.  The compile and argument
checks run without a GPU; the rest under `pytest -m gpu`."""
import json
import os
import subprocess

import pytest

from test_arena_cpu import BUILD, ROOT, gxx


def build_probe():
    return gxx(os.path.join(ROOT, "tests", "cpp", "policy_facade.cpp"), os.path.join(BUILD, "policy_facade"))


def build_train_example():
    return gxx(os.path.join(ROOT, "examples", "train_selfplay.cpp"), os.path.join(BUILD, "train_selfplay_policy"))


def build_arena_example():
    return gxx(os.path.join(ROOT, "examples", "arena.cpp"), os.path.join(BUILD, "arena_policy"))


def test_probe_and_examples_compile_and_the_example_checks_its_arguments():
    """xq::Policy, xq::ChessAI::setPolicy / setEpsilon and xq::Arena::setTemperature with plain g++ (no HIP headers)"""
    assert os.path.exists(build_probe()) and os.path.exists(build_arena_example())
    exe = build_train_example()
    for bad, word in (("policy=softmax", "policy="), ("policy=boltzmann:", "policy="), ("policy=boltzmann:hot", "policy="),
                      ("policy=boltzmann:1x", "policy="), ("eps=1.5", "eps="), ("eps=", "eps="), ("eps=-0.1", "eps="), ("eps=nan", "eps=")):
        out = subprocess.run([exe, "1", "m.bin", "1", bad], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and word in out.stderr, (bad, out.returncode, out.stderr)


@pytest.mark.gpu
def test_facade_carries_policy_and_epsilon_onto_the_trainer(tmp_path):
    exe = build_probe()
    out = subprocess.run([exe, "64", "40", "7", str(tmp_path / "m.bin")], check=True, capture_output=True, text=True, cwd=str(tmp_path),
                         timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    print(r)
    assert r["greedy_before"] == 1 and r["setter_refusals"] == 10 and r["unchanged"] == 1 and r["kept"] == 1
    assert r["train_refused"] == 1 and r["episode_refused"] == 1 and r["step_refused"] == 1 and r["selfplay_refused"] == 1
    assert r["move_refused"] == 1 and r["move_allowed"] == 1
    assert (r["base_kind"], r["base_eps"]) == (0, 0.1) and r["base_finite"] == 1
    # epsilon 0.1 of the reference: about a tenth of the plies explore (binomial, > 6 sigma either way)
    assert 0.07 * r["base_steps"] < r["base_explored"] < 0.13 * r["base_steps"], r
    assert (r["soft_kind"], r["soft_temp"], r["soft_eps"], r["soft_explored"]) == (1, 0.5, 0.0, 0) and r["soft_updates"] > 0
    assert (r["hard_kind"], r["hard_eps"], r["hard_explored"]) == (0, 0.0, 0)
    assert r["soft_finite"] == 1 and r["hard_finite"] == 1
    assert r["soft_vs_hard"] > 0 and r["base_vs_hard"] > 0          # both settings reach the trainer: other games, other parameters
    assert r["arena_t0"] == [0, 0] and r["arena_t1"] == [0.5, 0] and r["arena_t2"] == [0.5, 0] and r["arena_refusals"] == 10
    # evaluateAgainst's temperature pair: (self, opponent) in that order, on both overloads
    assert r["opp_temp_ignored"] == 1 and r["self_temp_moves"] == 1 and r["file_temp_moves"] == 1 and r["search_temp_refused"] == 1
    assert r["eval_refused"] == 1


@pytest.mark.gpu
def test_examples_take_the_new_arguments(tmp_path):
    exe = build_train_example()
    model = tmp_path / "m.bin"
    args = [exe, "64", str(model), "64", "--hidden", "64,64", "--replay", "1024", "--minibatch", "64", "--save-every", "0", "--seed", "7"]
    on = subprocess.run(args + ["policy=boltzmann:0.5", "eps=0", "--json"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    print(on.stdout[-1500:], on.stderr[-1500:])
    assert on.returncode == 0
    r = json.loads(on.stdout.strip().splitlines()[-1])
    assert (r["policy"], r["temperature"], r["epsilon"], r["explored_plies"]) == ("boltzmann", 0.5, 0.0, 0) and model.stat().st_size > 0
    txt = subprocess.run(args + ["policy=boltzmann:0.5"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert txt.returncode == 0 and "policy: boltzmann" in txt.stdout
    off = subprocess.run(args + ["policy=greedy", "eps=0.25", "--json"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    r = json.loads(off.stdout.strip().splitlines()[-1])
    assert (r["policy"], r["epsilon"]) == ("greedy", 0.25) and 0.15 * r["env_steps"] < r["explored_plies"] < 0.35 * r["env_steps"]
    # a temperature outside [1e-3, 1e3] is the facade's to refuse; the sequential loop keeps the reference's selectAction
    cold = subprocess.run(args + ["policy=boltzmann:0"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert cold.returncode == 1 and "setPolicy" in cold.stderr
    seq = subprocess.run([exe, "1", str(model), "1", "policy=boltzmann:1"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert seq.returncode == 1 and "Policy::boltzmann" in seq.stderr
    # the arena example: one model against itself — greedy twins score exactly one half, a temperature on A alone moves the games
    arena = build_arena_example()
    base = [arena, str(model), str(model), "32", "--seed", "3", "--opening", "4", "--json"]
    a = json.loads(subprocess.run(base, check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1])
    b = json.loads(subprocess.run(base + ["--temp-a", "1.0"], check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1])
    assert a["games"] == b["games"] == 64
    assert (a["plies"], a["wins"], a["draws"], a["losses"]) != (b["plies"], b["wins"], b["draws"], b["losses"]) or a["causes"] != b["causes"]
    bad = subprocess.run(base + ["--temp-a", "5000"], capture_output=True, text=True, timeout=300)
    assert bad.returncode == 1
