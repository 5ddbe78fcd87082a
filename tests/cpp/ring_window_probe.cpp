// ring_window_probe — walks cn_chess_ai_amd/csrc/xq_ring_window.h the way xq_trainer.hip uses it, over every small ring, and prints the
// plan of every iteration; tests/test_ring_window_cpu.py compares the lines with a simulated ring.  Plain C++17, links against nothing.
//
// One line per iteration:
//   cap games plies n_step prioritized order it | size write_pos inflight (as learn_grads finds them) | join_first play_first
//   sample readable excluded | first-tree rebuild (learn_grads without a tree) | learn_apply's rebuild     — a span is "first count",
//   a rebuild is "retire tree hold", a rebuild that does not happen is all -1
// order 0: learn_grads, collects, learn_apply (overlapped); 1: collects, learn_grads, learn_apply (overlapped); 2: the same, one stream
#include "../../cn_chess_ai_amd/csrc/xq_ring_window.h"

#include <cstdio>

using namespace xq;

static void print(RingSpan s) { std::printf(" %d %d", s.first, s.count); }
static void print(const RebuildPlan* p) {
    const RingSpan none{-1, -1};
    print(p ? p->retire : none); print(p ? p->tree : none); print(p ? p->hold : none);
}

static void walk(int cap, int games, int plies, int n_step, bool prioritized, int order) {
    const bool overlap = order != 2;
    RingState ring{0, 0, cap};
    RingSpan tree;
    bool tree_ready = false;
    const int iters = 3 * cap / games + 4;
    for (int it = 0; it < iters; ++it) {
        int inflight = 0, prepaid = 0;
        auto collects = [&] {                       // xq_trainer_collect x plies
            for (int c = 0; c < plies; ++c) {
                if (prepaid > 0) { prepaid--; continue; }
                ring = ring_after(ring, games);
                if (overlap) inflight += games;
            }
        };
        if (order != 0) collects();
        // xq_trainer_learn_grads
        std::printf("%d %d %d %d %d %d %d | %d %d %d |", cap, games, plies, n_step, (int)prioritized, order, it, ring.size, ring.write_pos, inflight);
        const IterationPlan p = plan_iteration({ring, games, plies, inflight, n_step, overlap, prioritized, tree_ready, tree});
        if (p.play_first) { collects(); prepaid = plies; }
        if (p.join_first && overlap) inflight = 0;
        RebuildPlan first_tree;
        const bool builds = p.join_first && prioritized;
        if (builds) {
            first_tree = plan_rebuild(ring, games, 0, n_step);
            tree = first_tree.tree;
            tree_ready = true;
        }
        std::printf(" %d %d", (int)p.join_first, (int)p.play_first);
        print(p.sample); print(p.readable);
        std::printf(" %d |", p.excluded);
        print(builds ? &first_tree : nullptr);
        std::printf(" |");
        if (order == 0) collects();
        // xq_trainer_learn_apply
        RebuildPlan next;
        if (prioritized) {
            next = plan_rebuild(ring, games, plies, n_step);
            tree = next.tree;
            tree_ready = true;
        }
        print(prioritized ? &next : nullptr);
        std::printf("\n");
    }
}

int main() {
    for (int cap = 1; cap <= 24; ++cap)
        for (int games = 1; games <= cap; ++games)
            for (int plies : {1, 2, 4})
                for (int n_step : {1, 2, 3, 5})
                    for (int prioritized = 0; prioritized < 2; ++prioritized)
                        for (int order = 0; order < 3; ++order) walk(cap, games, plies, n_step, prioritized != 0, order);
    return 0;
}
