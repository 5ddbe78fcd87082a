// xq_ring_window.h — which slots of the replay ring a training iteration may sample, which an n-step chain may read and which a tree
// rebuild retires and holds: the one statement of the trainer's window rule (DESIGN.md §4 "Ring windows").  Host-only integer arithmetic
// in plain C++17 — no HIP, no handle — so that a stand-alone program can walk it on the CPU (tests/cpp/ring_window_probe.cpp).
#pragma once

#include <algorithm>

namespace xq {

// `count` slots in age order (oldest first) from slot `first`, wrapping at the ring's capacity
struct RingSpan {
    int first = 0, count = 0;
    bool inside(int cap) const { return first >= 0 && first < cap && count >= 0 && count <= cap; }
};
// the ring's counters: filled slots, the slot the next write goes to, capacity (size < cap implies write_pos == size)
struct RingState { int size, write_pos, cap; };
inline RingState ring_after(RingState r, long long n) { return {(int)std::min<long long>(r.cap, r.size + n), (int)((r.write_pos + n) % r.cap), r.cap}; }
inline RingSpan ring_filled(RingState r) { return {r.size < r.cap ? 0 : r.write_pos, r.size}; }      // the filled ring

// s without its newest k slots ...
inline RingSpan span_cut(RingSpan s, long long k) { return {s.first, (int)std::max<long long>(0, s.count - k)}; }
// ... unless that leaves nothing: then s as it is (the first iterations of a run; the chains that reach past it are dead rows)
inline RingSpan span_cut_unless_empty(RingSpan s, long long k) { return s.count - k > 0 ? span_cut(s, k) : s; }
// ... and what span_cut_unless_empty took away, as a span of its own (nothing: {0, 0})
inline RingSpan span_held(RingSpan s, long long k, int cap) {
    const int h = s.count - span_cut_unless_empty(s, k).count;
    return h > 0 ? RingSpan{(int)(((long long)s.first + s.count - h) % cap), h} : RingSpan{};
}

// The filled slots that the next m writes from write_pos leave alone: the filled ring after those writes, without them.  The uniform
// overlap window, the range that goes with the prioritized tree and (what is missing from it) the retired slots are this one set
inline RingSpan ring_kept(RingState r, long long m) {
    const int w = (int)std::min<long long>(m, r.cap);            // (more writes than slots rewrite every slot)
    return span_cut(ring_filled(ring_after(r, w)), w);
}
// the slots those writes go to, once they reach filled ones — before that they are fresh slots of priority 0, and nothing is retired
inline RingSpan ring_retired(RingState r, long long m) { return {r.write_pos, r.size + m > r.cap ? (int)std::min<long long>(m, r.cap) : 0}; }

// ---- one iteration of the trainer ------------------------------------------------------------------------------------------------
struct IterationIn {
    RingState ring;
    int n_games, plies, inflight, n_step;   // plies per update; ring slots written by this iteration's collects so far (overlap only)
    bool overlap, prioritized, tree_ready;
    RingSpan tree;                          // prioritized, tree_ready: the range that goes with the tree (RebuildPlan::tree)
};
struct IterationPlan {
    bool join_first = false;            // the iteration's plies come before the draw: the collects in flight are waited for ...
    bool play_first = false;            // ... and with none in flight and nothing to learn from, the trainer plays them itself
    RingSpan sample;                    // the slots the minibatch is drawn from
    RingSpan readable{0, -1};           // n_step > 1: the slots a chain may read (count < 0: the ring's default, not narrowed)
    int excluded = 0;                   // the slots from write_pos - inflight that the draw leaves to the collects running beside it
};

inline IterationPlan plan_iteration(const IterationIn& in) {
    IterationPlan p;
    const int played = in.plies * in.n_games, m = in.inflight > 0 ? in.inflight : played;
    RingState r = in.ring;
    RingSpan window = in.tree;
    if (in.prioritized) {               // the tree of the last learn_apply, or none yet: built from the ring as it stands, played if empty
        p.join_first = !in.tree_ready;
        p.play_first = p.join_first && in.inflight == 0 && r.size == 0;
        p.excluded = in.tree_ready ? played : 0;
    } else if (in.overlap) {
        // the ring minus the slots this iteration's collects write: its newest `inflight` when they are queued already, else the next
        // `played` from write_pos.  Nothing older than this iteration's plies (the first iteration; played >= cap: every one): plies first
        window = in.inflight > 0 ? span_cut(ring_filled(r), m) : ring_kept(r, m);
        p.join_first = window.count <= 0;
        p.play_first = p.join_first && in.inflight == 0;
        p.excluded = p.join_first ? 0 : m;
    }
    if (p.play_first) r = ring_after(r, played);
    const bool whole = !in.prioritized && (!in.overlap || p.join_first);
    if (whole || (in.prioritized && !in.tree_ready)) window = ring_filled(r);
    p.sample = span_cut_unless_empty(window, (long long)(in.n_step - 1) * in.n_games);       // (the newest chains are not complete yet)
    if (in.n_step > 1) p.readable = window;
    else if (whole) p.sample.first = 0;     // the plain draw numbers the whole ring from slot 0 (xq_replay_sample): the same set
    return p;
}

// ---- the tree a prioritized learn_apply builds for the next iteration (plies = 0: the first tree, from the ring as it stands) -----
struct RebuildPlan { RingSpan retire, tree, hold; };   // out for good; the range that goes with the tree; out of this tree only
inline RebuildPlan plan_rebuild(RingState r, int n_games, int plies, int n_step) {
    const RingSpan tree = ring_kept(r, (long long)plies * n_games);
    return {ring_retired(r, (long long)plies * n_games), tree, span_held(tree, (long long)(n_step - 1) * n_games, r.cap)};
}

}  // namespace xq
