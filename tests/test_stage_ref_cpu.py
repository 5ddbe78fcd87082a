"""CPU checks of tests/stage_ref.py (not gpu), the composition the staging-matrix test holds the device against: with one stage on it
is that stage's own reference, and mirror and colour swap give the same batch in either order."""
import numpy as np
import pytest

import colour_swap_ref as cr
import mirror_ref as mr
import nstep_ref as nr
import stage_ref as sr
import view_ref as vr

SEED = 0x5EED0123456789
GAMMA = 0.97
BATCH_KEYS = ("boards", "next_boards", "action", "reward", "done", "slot", "first_slot", "last_slot")


def ring(name):
    fx = nr.named_fixture(name)
    rng = np.random.default_rng(fx["cap"])
    fx["next_player"] = rng.integers(0, 2, fx["cap"]).astype(np.uint8)
    fx["mover"] = np.where(rng.random(fx["cap"]) < 0.5, 1 - fx["next_player"], fx["next_player"]).astype(np.uint8)
    return fx


def draws(fx):
    rng = np.random.default_rng(7)
    return [nr.all_slots(fx), nr.filled_slots(fx), rng.integers(0, fx["size"], 65).astype(np.int32)]


def own_columns(got, fx, slots):
    """what no transform touches: reward, done and the slot columns of a one-step batch"""
    assert np.array_equal(got["reward"], fx["R"][slots]) and np.array_equal(got["done"], fx["D"][slots])
    for k in ("slot", "first_slot", "last_slot"):
        assert np.array_equal(got[k], slots), k


@pytest.mark.parametrize("name", sorted(nr.FIXTURES))
def test_one_stage_on_is_that_stages_own_reference(name):
    fx = ring(name)
    n = nr.FIXTURES[name][3]
    for slots in draws(fx):
        rows = len(slots)
        # nothing on: the ring's rows
        got = sr.stage(fx, slots, SEED, GAMMA)
        assert np.array_equal(got["boards"], fx["S"][slots]) and np.array_equal(got["next_boards"], fx["S2"][slots])
        assert np.array_equal(got["action"], fx["A"][slots]) and got["nstep"] is None and got["next_player"] is None
        assert all(got[k] is None for k in ("mirror_flags", "colour_swap_flags", "flag_s", "flag_next"))
        own_columns(got, fx, slots)
        # the assembly
        got = sr.stage(fx, slots, SEED, GAMMA, n_step=n, legal=True)
        ref = nr.assemble(fx["A"], fx["R"], fx["D"], fx["cap"], slots, n, fx["stride"], GAMMA, *nr.readable(fx["cap"], fx["size"], fx["write_pos"]))
        for k, want in zip(("boards", "action", "reward", "done", "next_boards"), nr.staged(fx, ref)):
            assert np.array_equal(got[k], want), k
        assert np.array_equal(got["first_slot"], ref["first_slot"]) and np.array_equal(got["last_slot"], ref["last_slot"])
        assert np.array_equal(got["slot"], slots) and np.array_equal(got["next_player"], fx["next_player"][ref["last_slot"]])
        if rows >= 37:
            assert (ref["last_slot"] != ref["first_slot"]).any()
        # the mirror
        got = sr.stage(fx, slots, SEED, GAMMA, mirror=0.5, calls=(3, 9), legal=True)
        want = mr.stage(fx, slots, 0.5, 3, SEED)
        for k in ("boards", "next_boards", "action", "slot"):
            assert np.array_equal(got[k], want[k]), k
        assert np.array_equal(got["mirror_flags"], want["flags"]) and np.array_equal(got["next_player"], fx["next_player"][slots])
        own_columns(got, fx, slots)
        # the colour swap, with and without the side
        for legal in (False, True):
            got = sr.stage(fx, slots, SEED, GAMMA, colour_swap=0.5, calls=(3, 9), legal=legal)
            want = cr.stage(fx, slots, 0.5, 9, SEED, side=fx["next_player"] if legal else None)
            for k in ("boards", "next_boards", "action", "slot"):
                assert np.array_equal(got[k], want[k]), k
            assert np.array_equal(got["colour_swap_flags"], want["flags"])
            assert np.array_equal(got["next_player"], want["next_player"]) if legal else got["next_player"] is None
            own_columns(got, fx, slots)
        # the view
        for legal in (False, True):
            got = sr.stage(fx, slots, SEED, GAMMA, view=True, legal=legal)
            want = vr.stage(fx, slots, fx["mover"], fx["next_player"])
            for k in ("boards", "next_boards", "action", "slot", "flag_s", "flag_next"):
                assert np.array_equal(got[k], want[k]), k
            assert np.array_equal(got["next_player"], want["next_player"]) if legal else got["next_player"] is None
            own_columns(got, fx, slots)


@pytest.mark.parametrize("name", sorted(nr.FIXTURES))
def test_mirror_and_colour_swap_commute(name):
    fx = ring(name)
    n = nr.FIXTURES[name][3]
    for slots in draws(fx):
        for n_step in (1, n):
            for prob in ((0.5, 0.5), (1.0, 0.5), (1.0, 1.0)):
                a, b = (sr.stage(fx, slots, SEED, GAMMA, n_step=n_step, mirror=prob[0], colour_swap=prob[1], legal=True, calls=(2, 5), order=o)
                        for o in (sr.ORDER, sr.ORDER[::-1]))
                for k in BATCH_KEYS + ("mirror_flags", "colour_swap_flags", "next_player"):
                    assert np.array_equal(a[k], b[k]), k
                both = (a["mirror_flags"] == 1) & (a["colour_swap_flags"] == 1)
                assert both.any()
                # a row that took both is neither transform alone
                m = sr.stage(fx, slots, SEED, GAMMA, n_step=n_step, mirror=prob[0], calls=(2, 5))
                c = sr.stage(fx, slots, SEED, GAMMA, n_step=n_step, colour_swap=prob[1], calls=(2, 5))
                assert not np.array_equal(a["boards"][both], m["boards"][both]) and not np.array_equal(a["boards"][both], c["boards"][both])


def test_view_with_colour_swap_is_refused():
    fx = ring("wrapped37")
    with pytest.raises(ValueError):
        sr.stage(fx, nr.all_slots(fx), SEED, GAMMA, colour_swap=0.5, view=True)
