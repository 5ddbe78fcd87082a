"""The staging pipeline of xq_dqn_td_grads_replay (DESIGN.md §4 "Staging pipeline") over every permitted combination of its stages —
`pytest -m gpu`: n-step assembly off / on, mirror off / on, then nothing, the colour swap or the mover view, under both bootstraps.  After
one step each case holds bit for bit: every column the read-backs of the stages that ran return against tests/stage_ref.py; the refusal
of every read-back whose stage did not run; the staging launches against the work model; Q(s, a), y and the parameters against a twin
handle that takes the reference's batch through the host entry point.  One prioritized case: the priorities land on the sampled slots."""
import numpy as np
import pytest

import nstep_ref as nr
import stage_ref as sr
from cn_chess_ai_amd import workmodel
from test_view_gpu import GAMMA, PER, RING_SEED, SMALL_NET, bits, filled, make_net, ring_fixture, same_step

pytestmark = pytest.mark.gpu

N_STEP = 3
STAGING = ("nstep_assemble", "mirror_stage", "colour_swap_stage", "mover_view_stage", "legal_side_stage", "per_writeback")
MATRIX = [(n, m, third, boot) for n in (1, N_STEP) for m in (False, True) for third in ("none", "colour_swap", "view") for boot in ("all", "legal")]
# (n_step, mirror, third transform, bootstrap, batch, probability of the random transforms)
CASES = [c + (65, 0.5) for c in MATRIX] + [(N_STEP, True, "colour_swap", "legal", 1, 1.0), (1, True, "view", "legal", 1, 1.0)]
REFUSALS = {"last_n_step": "an n-step", "last_mirror": "a mirror-mode", "last_colour_swap": "a colour-swap-mode", "last_view": "a view-mode"}


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


def configure(a, rp, fx, n_step, mirror, third, prob):
    if third == "view":
        a.set_view("mover")
    if n_step > 1:
        rp.set_n_step(n_step, fx["stride"])
    if mirror:
        rp.set_mirror(prob)
    if third == "colour_swap":
        rp.set_colour_swap(prob)


def reference(fx, slots, n_step, mirror, third, legal, prob):
    return sr.stage(fx, slots, RING_SEED, GAMMA, n_step=n_step, mirror=prob if mirror else 0.0,
                    colour_swap=prob if third == "colour_swap" else 0.0, view=third == "view", legal=legal)


def staging_launches(d):
    return {s["name"]: s["launches"] for s in d.kernel_stats() if s["name"] in STAGING}


def model_launches(batch, n_step, mirror, third, boot, prioritized=False):
    work = workmodel.step_work(SMALL_NET, batch, 64, n_step=n_step, mirror=mirror, bootstrap=boot, colour_swap=third == "colour_swap",
                               view=third == "view", prioritized=prioritized)
    return {k: 1 for k in work if k in STAGING}


def assert_read_backs(xq, d, want, rows, n_step, mirror, third, legal):
    ran = {"last_n_step": n_step > 1, "last_mirror": mirror, "last_colour_swap": third == "colour_swap", "last_view": third == "view"}
    for name, what in REFUSALS.items():
        if not ran[name]:
            with pytest.raises(xq.XqError) as e:
                getattr(d, name)(rows)
            assert e.value.code == 2 and f"xq_dqn_{name}: the last TD step was not {what} one" in str(e.value)
    batch_cols = ("boards", "next_boards", "action", "slot")
    if ran["last_n_step"]:
        got, ref = d.last_n_step(rows), want["nstep"]
        for k in ("reward", "done", "first_slot", "last_slot", "action"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["steps"], ref["steps"])
        if rows > 1:
            assert (ref["last_slot"] != ref["first_slot"]).any()
    if ran["last_mirror"]:
        got = d.last_mirror(rows)
        assert np.array_equal(got["flags"], want["mirror_flags"])
        for k in batch_cols:
            assert np.array_equal(got[k], want[k]), k
    if ran["last_colour_swap"]:
        got = d.last_colour_swap(rows, next_player=legal)
        assert np.array_equal(got["flags"], want["colour_swap_flags"])
        for k in batch_cols + (("next_player",) if legal else ()):
            assert np.array_equal(got[k], want[k]), k
        if not legal:
            with pytest.raises(xq.XqError) as e:
                d.last_colour_swap(rows, next_player=True)
            assert e.value.code == 1 and "next_player asked" in str(e.value)
    if ran["last_view"]:
        got = d.last_view(rows)
        for k in batch_cols + ("flag_s", "flag_next"):
            assert np.array_equal(got[k], want[k]), k


@pytest.mark.parametrize("n_step,mirror,third,boot,batch,prob", CASES)
def test_every_combination_stages_the_reference_batch_and_steps_on_it(xq, golden_dir, n_step, mirror, third, boot, batch, prob):
    lr, legal = 0.05, boot == "legal"
    fx = ring_fixture(golden_dir)
    rp = filled(xq, fx)
    twin_gamma = float(nr.discounts(GAMMA, n_step)[n_step]) if n_step > 1 else GAMMA
    a, b = make_net(xq, legal=legal), make_net(xq, legal=legal, gamma=twin_gamma)
    try:
        configure(a, rp, fx, n_step, mirror, third, prob)
        slots = rp.sample(batch)
        want = reference(fx, slots, n_step, mirror, third, legal, prob)
        for flags in (want["mirror_flags"], want["colour_swap_flags"]):      # the seed shows both values of every random flag
            assert flags is None or (set(np.unique(flags)) == {0, 1} if batch > 1 else flags.all())
        a.kernel_stats(2)
        a.td_grads_replay(rp, batch, td_net=2)
        a.apply_grads(lr, 1.0 / batch)
        assert staging_launches(a) == model_launches(batch, n_step, mirror, third, boot)
        a.kernel_stats(0)
        assert_read_backs(xq, a, want, batch, n_step, mirror, third, legal)
        b.td_update(want["boards"], want["next_boards"], want["action"], want["reward"], want["done"], td_net=2, learning_rate=lr,
                    grad_scale=1.0 / batch, next_player=want["next_player"])
        same_step(a, b, batch)
    finally:
        a.close(); b.close(); rp.close()


def test_prioritized_staged_step_writes_its_priorities_to_the_sampled_slots(xq, golden_dir):
    batch, n_step, prob = 65, N_STEP, 0.5
    fx = ring_fixture(golden_dir)
    rp = filled(xq, fx, per=PER)
    a, b = make_net(xq), make_net(xq, gamma=float(nr.discounts(GAMMA, n_step)[n_step]))
    try:
        configure(a, rp, fx, n_step, True, "view", prob)
        rp.set_priorities(np.random.default_rng(5).uniform(1.0, 2.0, size=fx["cap"]).astype(np.float32))
        rp.per_rebuild()
        slots, _ = rp.sample_prioritized(batch)
        before = rp.get_priorities(0, fx["cap"])
        a.kernel_stats(2)
        a.td_grads_replay(rp, batch, td_net=2)
        a.apply_grads(0.0, 1.0)
        assert staging_launches(a) == model_launches(batch, n_step, True, "view", "all", prioritized=True)
        a.kernel_stats(0)
        want = reference(fx, slots, n_step, True, "view", False, prob)
        assert_read_backs(xq, a, want, batch, n_step, True, "view", False)
        assert (want["last_slot"] != want["first_slot"]).any() and np.array_equal(want["first_slot"], slots)
        qa, ya = a.last_td_values(batch)
        # the host step has no importance weights: targets and Q(s, a) agree bit for bit, and the priorities follow them
        qb, yb = b.td_update(want["boards"], want["next_boards"], want["action"], want["reward"], want["done"], td_net=2, learning_rate=0.0)
        assert np.array_equal(bits(qa), bits(qb)) and np.array_equal(bits(ya), bits(yb))
        after = rp.get_priorities(0, fx["cap"])
        live = want["action"] >= 0
        expect = (np.abs(qa.astype(np.float64) - ya) + PER[2]) ** PER[0]
        for s in set(int(x) for x in slots[live]):
            dup = [j for j in range(batch) if slots[j] == s and live[j]]
            assert min(abs(after[s] / expect[j] - 1) for j in dup) < 2e-5        # (fp32 powf against fp64: test_view_gpu's bound)
        rest = np.setdiff1d(np.arange(fx["cap"]), slots[live])
        assert np.array_equal(after[rest], before[rest]) and live.any()
    finally:
        a.close(); b.close(); rp.close()
