// The search player through the header-only facade (tests/test_search_gpu.py): argv = pairs, seed, depth.
// Prints one JSON line: the summary of Player::search(depth) against Player::random(), the same through ChessAI::evaluateAgainst with
// an untrained net against the search, and VecEnv::search on the start position.
#include <cstdio>
#include <cstdlib>

#include "xq/xq.hpp"

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int pairs = std::atoi(argv[1]), depth = std::atoi(argv[3]);
    const uint64_t seed = std::strtoull(argv[2], nullptr, 10);
    xq::Arena arena(pairs, seed);
    arena.run(xq::Player::search(depth, 0.1), xq::Player::random());
    const xq::ArenaSummary s = arena.summary();
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    ai.initializeDQN();
    const xq::ArenaSummary t = ai.evaluateAgainst(depth, pairs, seed);
    xq::VecEnv env(1);
    const xq::VecEnv::SearchResult r = env.search(depth);
    std::printf("{\"wins\": %d, \"draws\": %d, \"losses\": %d, \"score\": %.9f, \"causes\": [%d, %d, %d, %d, %d], "
                "\"net_score\": %.9f, \"net_games\": %d, \"start_count\": %d, \"start_best\": %d, \"start_value0\": %d}\n",
                s.wins, s.draws, s.losses, s.score, s.causes[0], s.causes[1], s.causes[2], s.causes[3], s.causes[4], t.score, t.scoredGames,
                r.counts[0], r.best[0], r.values[0]);
    return 0;
}
