// Versus training through the header-only facade (tests/test_versus_gpu.py): argv = games, episodes, seed, depth.
// Prints one JSON line: whether the sequential loop refused the opponent (std::logic_error), then what the batched train() against
// Player::search(depth) did: env steps, episodes, and the learner's wins, draws, losses and games ended.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "xq/xq.hpp"

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]), depth = std::atoi(argv[4]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    ai.setOpponent(xq::Player::search(depth, 0.1));
    ai.setParallelGames(1);
    int refused = 0;
    try {
        ai.train(1);
    } catch (const std::logic_error&) {
        refused = 1;
    }
    ai.setParallelGames(games);
    ai.setBatchSeed(seed);
    ai.train(episodes);
    const xq::ChessAI::TrainStats s = ai.lastTrainStats();
    std::printf("{\"refused\": %d, \"env_steps\": %llu, \"episodes\": %llu, \"wins\": %llu, \"draws\": %llu, \"losses\": %llu, \"ended\": %llu}\n",
                refused, (unsigned long long)s.envSteps, (unsigned long long)s.episodes, (unsigned long long)s.versus[0],
                (unsigned long long)s.versus[1], (unsigned long long)s.versus[2], (unsigned long long)s.versus[3]);
    return 0;
}
