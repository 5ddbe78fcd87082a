// n-step returns through the header-only facade (tests/test_nstep_gpu.py): argv = games, episodes, seed, n.
// Prints one JSON line: what xq::ReplayBuffer::nStep() reports around setNStep, whether n = 9 and a chain that does not fit the ring were
// refused (std::invalid_argument), and for a batched train() with a replay ring under xq::ChessAI::setNStep(n) and under the default:
// the n-step setting of the trainer's ring as the run ended and the updates done.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static int train(xq::ChessAI& ai, int games, int episodes, uint64_t seed, unsigned long long* updates) {
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setParallelGames(games);
    ai.setReplay(games * 16, games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    *updates = ai.lastTrainStats().updates;
    return ai.lastTrainStats().nStep;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]), n = std::atoi(argv[4]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    xq::ReplayBuffer ring(64, seed);
    const int ringBefore = ring.nStep();
    ring.setNStep(n, 4);
    const int ringAfter = ring.nStep();
    int nineRefused = 0, longRefused = 0, aiNineRefused = 0;
    try { ring.setNStep(9, 1); } catch (const std::invalid_argument&) { nineRefused = 1; }
    try { ring.setNStep(3, 32); } catch (const std::invalid_argument&) { longRefused = 1; }
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    try { ai.setNStep(9); } catch (const std::invalid_argument&) { aiNineRefused = 1; }
    unsigned long long u1 = 0, un = 0;
    const int plain = train(ai, games, episodes, seed, &u1);
    ai.setNStep(n);
    const int stepped = train(ai, games, episodes, seed, &un);
    std::printf("{\"ring_before\": %d, \"ring_after\": %d, \"nine_refused\": %d, \"long_refused\": %d, \"ai_nine_refused\": %d, "
                "\"plain_n\": %d, \"plain_updates\": %llu, \"stepped_n\": %d, \"stepped_updates\": %llu}\n",
                ringBefore, ringAfter, nineRefused, longRefused, aiNineRefused, plain, u1, stepped, un);
    return 0;
}
