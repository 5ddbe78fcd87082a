"""The env's ring of finished-episode records past its capacity (`pytest -m gpu`): xq_env_drain_episodes after more than ep_cap episodes
without a drain, in pieces across the ring's wrap point, and at its argument edges.

1024 games of random self-play: ep_cap = max(4096, 4 * n_games) = 4096.  What a drain must return is known from the step results of the
same env, ply by ply; inside one ply the order of the records is that of device atomics, so plies are compared as sets."""
import ctypes as C
import time
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_GAMES, EP_CAP, SEED, FIRST_ID = 1024, 4096, 77, 5000
MAX_PLIES = 1200          # test_selfplay_full_size_invariants bounds the mean game at 120..190 plies: 1024 games end 5096 times well before


@pytest.fixture(scope="module")
def xq():
    import cn_chess_ai_amd as m
    assert m._capi.device_count() > 0
    return m


class Game:
    """an env beside the records its plies must have produced"""

    def __init__(self, xq):
        self.env = xq.VecEnv(N_GAMES, seed=SEED, first_game_id=FIRST_ID)
        self.count = np.zeros(N_GAMES, np.int64)          # finished episodes per game slot
        self.plies = []                                   # per ply: the list of its records
        self.t0 = time.perf_counter()

    def restart(self):
        self.env.reset()
        self.count[:] = 0
        self.plies = []

    def ply(self):
        res = self.env.selfplay_step(None)
        ended = np.nonzero(res["terminated"])[0]
        self.count[ended] += 1
        self.plies.append([(FIRST_ID + int(g), int(self.count[g]), int(res["red_score"][g]), int(res["black_score"][g]),
                            int(res["move_count"][g]), int(res["winner"][g]), int(res["action"][g] < 0)) for g in ended])

    def play_until(self, episodes):
        """plies until at least `episodes` have finished since the start (or restart); fails when MAX_PLIES do not get there"""
        while self.total() < episodes:
            assert len(self.plies) < MAX_PLIES, "only %d episodes after %d plies" % (self.total(), len(self.plies))
            self.ply()

    def total(self):
        return sum(len(p) for p in self.plies)

    def close(self):
        self.env.close()


def tuples(rec):
    return [(int(e["game_id"]), int(e["episode"]), int(e["red_score"]), int(e["black_score"]), int(e["move_count"]), int(e["winner"]),
             int(e["reserved"])) for e in rec]


def check_run(game, got, first):
    """`got`: drained records that must be episodes number first .. first + len(got) - 1 (0-based, in order of completion) of `game`:
    whole plies as multisets, a ply cut at either end as a subset of the right size; no (game_id, episode) twice; ply of completion
    non-decreasing along the array"""
    assert len({g[:2] for g in got}) == len(got), "a (game_id, episode) pair twice"
    ply_of = {r[:2]: t for t, p in enumerate(game.plies) for r in p}
    at = [ply_of[g[:2]] for g in got]                     # (KeyError: a record no ply produced)
    assert all(a <= b for a, b in zip(at, at[1:])), "not oldest first"
    bounds = np.cumsum([0] + [len(p) for p in game.plies])
    last = first + len(got)
    for t, p in enumerate(game.plies):
        lo, hi = max(int(bounds[t]), first), min(int(bounds[t + 1]), last)
        if hi <= lo:
            continue
        part = Counter(got[lo - first:hi - first])
        if hi - lo == len(p):
            assert part == Counter(p), "ply %d" % t
        else:
            assert not part - Counter(p) and sum(part.values()) == hi - lo, "cut ply %d" % t


def drain_raw(xq, env, records, max_records):
    """xq_env_drain_episodes with any pointer (None = NULL) -> (n_out, total)"""
    n, total = C.c_int32(-1), C.c_uint64(99)
    xq._capi.call("xq_env_drain_episodes", env.handle, records, int(max_records), C.byref(n), C.byref(total))
    return n.value, total.value


def test_overflow_keeps_the_newest_ep_cap_records(xq):
    g = Game(xq)
    g.play_until(EP_CAP + 1000)
    total = g.total()
    assert g.env.counters()["episodes"] == total >= EP_CAP + 1000
    bounds = np.cumsum([0] + [len(p) for p in g.plies])
    overflow_ply = int(np.searchsorted(bounds, EP_CAP, side="right"))         # the first ply behind which more than ep_cap had finished
    rec, tot = g.env.drain_episodes(2 * EP_CAP)
    assert tot == total and len(rec) == EP_CAP
    check_run(g, tuples(rec), total - EP_CAP)
    rec2, tot2 = g.env.drain_episodes(2 * EP_CAP)
    assert len(rec2) == 0 and tot2 == total
    # ... and the ring goes on from there
    g.ply(); g.ply(); g.ply()
    rec3, tot3 = g.env.drain_episodes(2 * EP_CAP)
    assert tot3 == g.total() and len(rec3) == tot3 - total
    check_run(g, tuples(rec3), total)
    print("episode ring: %d episodes after %d plies (more than ep_cap = %d from ply %d on), %.2f s"
          % (total, len(g.plies) - 3, EP_CAP, overflow_ply, time.perf_counter() - g.t0))
    g.close()


def test_partial_drains_across_the_wrap_point(xq):
    """the pending run straddles index ep_cap - 1; max_records 7, then 1000 (that call copies the two sides of the wrap point), then the rest"""
    g = Game(xq)
    g.play_until(EP_CAP - 500)
    rec, first = g.env.drain_episodes(2 * EP_CAP)
    assert len(rec) == first == g.total()
    check_run(g, tuples(rec), 0)
    assert first + 7 < EP_CAP <= first + 1007, first        # the second drain below crosses the wrap point
    g.play_until(first + 1107)
    total = g.total()
    assert total - first <= EP_CAP                          # nothing is lost
    parts = []
    for max_records in (7, 1000, 2 * EP_CAP):
        rec, tot = g.env.drain_episodes(max_records)
        assert tot == total and len(rec) == min(max_records, total - first - sum(len(p) for p in parts))
        parts.append(tuples(rec))
    assert [len(p) for p in parts[:2]] == [7, 1000] and len(parts[2]) >= 100
    check_run(g, parts[0] + parts[1] + parts[2], first)
    assert len(g.env.drain_episodes(16)[0]) == 0
    print("partial drains: %d drained first, then 7 + 1000 + %d across index %d, %.2f s" % (first, len(parts[2]), EP_CAP - 1, time.perf_counter() - g.t0))
    g.close()


def test_argument_edges_and_reset(xq):
    from cn_chess_ai_amd._capi import EpisodeRecord
    g = Game(xq)
    g.play_until(300)
    total = g.total()
    buf = (EpisodeRecord * 8)()
    assert drain_raw(xq, g.env, buf, 0) == (0, total)                   # max_records = 0
    assert drain_raw(xq, g.env, None, 8) == (0, total)                  # no buffer
    assert drain_raw(xq, g.env, None, 0) == (0, total)
    rec, tot = g.env.drain_episodes(2 * EP_CAP)                         # ... and not one record was lost to them
    assert tot == total == len(rec)
    check_run(g, tuples(rec), 0)
    # past the capacity the same calls drop what was overwritten, no more: the next drain has the newest ep_cap records
    g.play_until(EP_CAP + 300)
    total = g.total()
    assert drain_raw(xq, g.env, buf, 0) == (0, total) and drain_raw(xq, g.env, None, 8) == (0, total)
    rec, tot = g.env.drain_episodes(2 * EP_CAP)
    assert tot == total and len(rec) == EP_CAP
    check_run(g, tuples(rec), total - EP_CAP)
    # xq_env_reset: nothing pending, the total and the episode numbers start again
    g.play_until(total + 50)
    g.restart()
    assert drain_raw(xq, g.env, buf, 8) == (0, 0)
    assert g.env.counters()["episodes"] == 0
    g.play_until(20)
    rec, tot = g.env.drain_episodes(2 * EP_CAP)
    assert tot == g.total() == len(rec)
    check_run(g, tuples(rec), 0)
    assert len(rec) >= 20 and (rec["episode"] == 1).sum() >= 1 and rec["episode"].min() == 1
    first_of_slot = {}
    for e in tuples(rec):
        first_of_slot.setdefault(e[0], e[1])
    assert set(first_of_slot.values()) == {1}                           # every slot's first record since the reset is its episode 1
    print("argument edges and reset: %.2f s" % (time.perf_counter() - g.t0))
    g.close()
