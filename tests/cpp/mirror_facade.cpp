// Mirror augmentation through the header-only facade (tests/test_mirror_gpu.py): argv = games, episodes, seed, prob.
// Prints one JSON line: what xq::ReplayBuffer::mirror() reports around setMirror, whether 1.5 and NaN were refused
// (std::invalid_argument), and for a batched train() with a replay ring under the default and under xq::ChessAI::setMirror(prob): the
// mirror probability of the trainer's ring as the run ended and the updates done.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static double train(xq::ChessAI& ai, int games, int episodes, uint64_t seed, unsigned long long* updates) {
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setParallelGames(games);
    ai.setReplay(games * 16, games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    *updates = ai.lastTrainStats().updates;
    return ai.lastTrainStats().mirror;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const double prob = std::atof(argv[4]);
    xq::ReplayBuffer ring(64, seed);
    const double ringBefore = ring.mirror();
    ring.setMirror(prob);
    const double ringAfter = ring.mirror();
    int bigRefused = 0, nanRefused = 0, aiBigRefused = 0, aiNanRefused = 0;
    try { ring.setMirror(1.5); } catch (const std::invalid_argument&) { bigRefused = 1; }
    try { ring.setMirror(std::nan("")); } catch (const std::invalid_argument&) { nanRefused = 1; }
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    try { ai.setMirror(-0.1); } catch (const std::invalid_argument&) { aiBigRefused = 1; }
    try { ai.setMirror(std::nan("")); } catch (const std::invalid_argument&) { aiNanRefused = 1; }
    const double aiBefore = ai.mirror();
    unsigned long long u0 = 0, u1 = 0;
    const double plain = train(ai, games, episodes, seed, &u0);
    ai.setMirror(prob);
    const double mirrored = train(ai, games, episodes, seed, &u1);
    std::printf("{\"ring_before\": %.17g, \"ring_after\": %.17g, \"big_refused\": %d, \"nan_refused\": %d, \"ai_neg_refused\": %d, "
                "\"ai_nan_refused\": %d, \"ai_before\": %.17g, \"ai_after\": %.17g, \"plain_mirror\": %.17g, \"plain_updates\": %llu, "
                "\"mirrored_mirror\": %.17g, \"mirrored_updates\": %llu}\n",
                ringBefore, ringAfter, bigRefused, nanRefused, aiBigRefused, aiNanRefused, aiBefore, ai.mirror(), plain, u0, mirrored, u1);
    return 0;
}
