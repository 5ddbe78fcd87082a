"""The zero-sum target through the C++ facade and the example (`pytest -m gpu`): tests/cpp/zero_sum_facade.cpp — xq::DQN::setZeroSum
round trip, TrainStats::zero_sum, the throws of the single-board loops, the conflict with setOpponent — and
examples/train_selfplay ... target=zerosum."""
import json
import subprocess

import pytest

from test_zero_sum_capi_cpu import build_example, build_zero_sum_facade_probe

pytestmark = pytest.mark.gpu


def test_facade_carries_zero_sum_onto_the_trainers_network():
    exe = build_zero_sum_facade_probe()
    out = subprocess.run([exe, "64", "40", "7"], check=True, capture_output=True, text=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["before"], r["after"], r["kept"], r["back"]) == (0, 1, 1, 0)
    assert (r["ai_before"], r["ai_after"]) == (0, 1)
    assert r["train_refused"] == 1 and r["episode_refused"] == 1 and r["step_refused"] == 1 and r["selfplay_refused"] == 1
    assert r["opponent_refused"] == 1 and r["zero_sum_refused"] == 1 and r["off_allowed"] == 1
    assert r["on_zero_sum"] == 1 and r["off_zero_sum"] == 0
    assert r["on_updates"] > 0 and r["off_updates"] > 0 and r["on_finite"] == 1 and r["off_finite"] == 1
    assert r["max_param_diff"] > 0


def test_example_trains_with_the_zero_sum_target(tmp_path):
    exe = build_example()
    model = tmp_path / "m.bin"
    args = [exe, "64", str(model), "64", "--hidden", "64,64", "--replay", "1024", "--minibatch", "64", "--save-every", "0", "--seed", "7"]
    on = subprocess.run(args + ["target=zerosum"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    print(on.stdout[-1500:], on.stderr[-1500:])
    assert on.returncode == 0 and "target: zero-sum" in on.stdout and model.stat().st_size > 0
    off = subprocess.run(args + ["target=reference"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert off.returncode == 0 and "target: zero-sum" not in off.stdout
    # the sequential loop is the reference's: it refuses
    seq = subprocess.run([exe, "1", str(model), "1", "target=zerosum"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert seq.returncode == 1 and "setZeroSum" in seq.stderr
