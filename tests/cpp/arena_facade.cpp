// ChessAI::evaluateAgainst through the header-only facade (tests/test_arena_gpu.py): argv = model A, model B | random, pairs, seed.
// Prints the summary as one JSON line.
#include <cstdio>
#include <cstdlib>

#include "xq/xq.hpp"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    ai.initializeDQN();
    ai.loadModel(argv[1]);
    const xq::ArenaSummary s = ai.evaluateAgainst(argv[2], std::atoi(argv[3]), std::strtoull(argv[4], nullptr, 10));
    std::printf("{\"wins\": %d, \"draws\": %d, \"losses\": %d, \"score\": %.9f, \"ci95\": [%.9f, %.9f], \"elo\": %.6f, "
                "\"causes\": [%d, %d, %d, %d, %d]}\n", s.wins, s.draws, s.losses, s.score, s.ciLow, s.ciHigh, s.elo,
                s.causes[0], s.causes[1], s.causes[2], s.causes[3], s.causes[4]);
    return 0;
}
