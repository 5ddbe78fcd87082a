"""cn_chess_ai_amd/csrc/xq_ring_window.h — which ring slots a training iteration samples, reads, retires and holds — walked across the
first wraps of every small ring on the CPU (tests/cpp/ring_window_probe.cpp, plain g++, once more under ASan + UBSan) and compared with
a simulated ring: an array that holds, per slot, the sequence number of the write that filled it.  Every set is read off that array by
brute force; a set the trainer needs must be one contiguous span in age order, and then (first, count) is compared.

Two spans have no single `first`, and the test says so where it compares them:
  * an empty span: only its count is compared.  With plies x games < capacity no sample, readable or tree span is empty from the
    iteration on at which learn_grads finds more than plies x games transitions in the ring — asserted below;
  * the whole ring drawn without n-step chains (one stream, or the plies played first): the plain draw numbers the slots from 0, as
    xq_replay_sample does, so `first` must be 0 and the SET is compared — it is the oldest slot's span too until the ring is full."""
import os
import subprocess

import pytest

from ring_window_ref import default_range, overlap_window, tree_range

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
SRC = os.path.join(ROOT, "tests", "cpp", "ring_window_probe.cpp")
N_STEPS = (1, 2, 3, 5)
DEFAULT = (0, -1)                     # IterationPlan::readable when the step does not narrow the ring's default


def build(name, *flags):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *flags, SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def lines():
    return subprocess.run([build("ring_window_probe", "-O1")], check=True, capture_output=True, text=True).stdout.splitlines()


@pytest.fixture(scope="module")
def plans(lines):
    out = {}
    for ln in lines:
        key, state, plan, first_tree, next_tree = ([int(x) for x in part.split()] for part in ln.split("|"))
        out[tuple(key)] = (state, plan, first_tree, next_tree)
    return out


def test_probe_is_clean_under_asan_and_ubsan(lines):
    exe = build("ring_window_probe_san", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.splitlines() == lines


# ---- the simulated ring ---------------------------------------------------------------------------------------------------------------
class Ring:
    def __init__(self, cap):
        self.cap, self.seq, self.n = cap, [None] * cap, 0

    def write(self, k):
        for _ in range(k):
            self.seq[self.n % self.cap] = self.n
            self.n += 1

    def filled(self):
        """filled slots, oldest first"""
        return sorted((s for s in range(self.cap) if self.seq[s] is not None), key=lambda s: self.seq[s])

    def next_positions(self, m):
        """the distinct slots the next m writes go to, in write order"""
        return list(dict.fromkeys((self.n + i) % self.cap for i in range(m)))


def span_of(slots, cap):
    """(first, count) of a set given oldest first — which must be one contiguous run of slots"""
    assert all(b == (a + 1) % cap for a, b in zip(slots, slots[1:])), slots
    return (slots[0] if slots else None), len(slots)


def same_span(got, slots, cap):
    first, count = span_of(slots, cap)
    return got[1] == count and (count == 0 or got[0] == first)          # an empty span: the count alone


def expand(span, cap):
    return [(span[0] + i) % cap for i in range(span[1])]


def cut_unless_empty(slots, k):
    return slots[:len(slots) - k] if len(slots) - k > 0 else slots


def newest(slots, k):
    return slots[len(slots) - k:] if k > 0 else []


def walk(plans, cap, games, plies, prioritized, order):
    ring, m, overlap = Ring(cap), plies * games, order != 2
    tree = None                                                       # prioritized: the slots in the tree, oldest first
    checked = 0
    for it in range(3 * cap // games + 4):
        written = []                                                  # the slots this iteration's collects write
        if order != 0:
            written = ring.next_positions(m)
            ring.write(m)
        inflight = m if order == 1 else 0
        size, total, filled0 = len(ring.filled()), ring.n, ring.filled()
        assert default_range(size, total, cap) == span_of(filled0, cap) or size == 0
        # ---- learn_grads: what the trainer's rule says, read off the ring ----
        join = play = whole = False
        if prioritized:
            join = tree is None
            play = join and inflight == 0 and size == 0
            excluded = 0 if join else m
        elif overlap:
            if order == 0:
                nxt = set(ring.next_positions(m))
                window = [s for s in filled0 if s not in nxt]
                ow = overlap_window(size, total, cap, m)
                assert (ow[1] <= 0 and not window) or ow == span_of(window, cap)
            else:
                window = [s for s in filled0 if ring.seq[s] < ring.n - m]
            join = whole = not window
            play = join and inflight == 0
            excluded = 0 if join else m
        else:
            whole, excluded = True, 0
        if play:
            written = ring.next_positions(m)
            ring.write(m)
        if prioritized and join:
            tree = ring.filled()
        base = tree if prioritized else ring.filled() if whole else window
        first_tree = tree if prioritized and join else None
        # ---- the collects that follow learn_grads, then learn_apply ----
        if order == 0 and not play:
            written = ring.next_positions(m)
            ring.write(m)
        size1, total1 = len(ring.filled()), ring.n
        nxt = ring.next_positions(m)
        retire = nxt if any(ring.seq[s] is not None for s in nxt) else []
        next_tree = [s for s in ring.filled() if s not in set(nxt)]
        if m <= cap:
            tr = tree_range(size1, total1, cap, m)
            assert tr[1] == len(next_tree) and (not next_tree or tr == span_of(next_tree, cap))
        # ---- against the header, for every chain length ----
        for n_step in N_STEPS:
            k = (n_step - 1) * games
            state, plan, got_first, got_next = plans[(cap, games, plies, n_step, int(prioritized), order, it)]
            assert state == [size, total % cap, inflight]
            g_join, g_play, g_sample, g_readable, g_excluded = plan[0], plan[1], plan[2:4], plan[4:6], plan[6]
            assert (g_join, g_play, g_excluded) == (int(join), int(play), excluded)
            sample = cut_unless_empty(base, k)
            if whole and n_step == 1:       # the plain draw's numbering (module docstring): from slot 0, the same set
                assert g_sample[0] == 0 and sorted(expand(g_sample, cap)) == sorted(sample)
                assert len(sample) == cap or same_span(g_sample, sample, cap)
            else:
                assert same_span(g_sample, sample, cap)
            assert tuple(g_readable) == DEFAULT if n_step == 1 else same_span(g_readable, base, cap)
            if overlap and not join:        # the draw and the chains stay clear of the slots the collects beside them write
                assert not set(written) & set(expand(g_sample, cap)) and not set(written) & set(expand(g_readable, cap) if n_step > 1 else [])
            for got, slots, retired in ((got_first, first_tree, []), (got_next, next_tree if prioritized else None, retire)):
                if slots is None:
                    assert got == [-1] * 6
                    continue
                assert same_span(got[0:2], retired, cap) and same_span(got[2:4], slots, cap)
                assert same_span(got[4:6], newest(slots, len(slots) - len(cut_unless_empty(slots, k))), cap)
            if m < cap and size > m:        # (module docstring) nothing the trainer draws or reads from is empty here
                assert g_sample[1] > 0 and (n_step == 1 or g_readable[1] > 0) and (not prioritized or got_next[3] > 0)
            checked += 1
        if prioritized:
            tree = next_tree
    assert ring.n >= 2 * cap                                          # every ring wraps at least twice
    return checked


@pytest.mark.parametrize("prioritized", [False, True])
@pytest.mark.parametrize("order", [0, 1, 2])
def test_every_small_ring_across_its_first_wraps(plans, prioritized, order):
    """capacity 1..24 x games 1..capacity x plies {1, 2, 4} x n_step {1, 2, 3, 5}; order 0: learn_grads first, 1: collects first (both
    overlapped), 2: collects first on one stream.  Includes every point with plies x games >= capacity"""
    checked = sum(walk(plans, cap, games, plies, prioritized, order)
                  for cap in range(1, 25) for games in range(1, cap + 1) for plies in (1, 2, 4))
    assert checked * 6 == len(plans)
