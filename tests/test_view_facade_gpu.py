"""The mover view through the C++ facade and the example (`pytest -m gpu`): tests/cpp/view_facade.cpp — xq::DQN::setView round trip,
TrainStats::view, the throws of the single-board paths, the conflict with setColourSwap — and examples/train_selfplay ... view=mover."""
import json
import subprocess

import pytest

from test_view_capi_cpu import build_example, build_view_facade_probe

pytestmark = pytest.mark.gpu


def test_facade_carries_the_view_onto_the_trainer():
    exe = build_view_facade_probe()
    out = subprocess.run([exe, "64", "40", "7"], check=True, capture_output=True, text=True, timeout=300).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert (r["before"], r["after"], r["kept"], r["back"]) == (0, 1, 1, 0)
    assert (r["ai_before"], r["ai_after"]) == (0, 1)
    assert r["train_refused"] == 1 and r["episode_refused"] == 1 and r["step_refused"] == 1 and r["selfplay_refused"] == 1
    assert r["move_refused"] == 1
    assert r["swap_refused"] == 1 and r["swap_off_allowed"] == 1 and r["view_refused"] == 1
    assert r["on_mover"] == 1 and r["off_mover"] == 0 and r["on_net_kept"] == 1 and r["off_net_kept"] == 1
    assert r["on_updates"] > 0 and r["off_updates"] > 0 and r["on_finite"] == 1 and r["off_finite"] == 1
    assert r["max_param_diff"] > 0


def test_example_trains_with_the_mover_view(tmp_path):
    exe = build_example()
    model = tmp_path / "m.bin"
    args = [exe, "64", str(model), "64", "--hidden", "64,64", "--replay", "1024", "--minibatch", "64", "--save-every", "0", "--seed", "7"]
    on = subprocess.run(args + ["view=mover", "target=zerosum", "bootstrap=legal"], capture_output=True, text=True, cwd=str(tmp_path),
                        timeout=300)
    print(on.stdout[-1500:], on.stderr[-1500:])
    assert on.returncode == 0 and "view: mover" in on.stdout and model.stat().st_size > 0
    off = subprocess.run(args + ["view=absolute"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert off.returncode == 0 and "view: mover" not in off.stdout
    # the colour swap and the view refuse each other; the sequential loop reads the absolute board
    both = subprocess.run(args + ["swap=0.5", "view=mover"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert both.returncode == 1 and "setColourSwap" in both.stderr
    seq = subprocess.run([exe, "1", str(model), "1", "view=mover"], capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert seq.returncode == 1 and "setView" in seq.stderr
