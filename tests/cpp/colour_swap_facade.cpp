// Colour-swap augmentation through the header-only facade (tests/test_colour_swap_gpu.py): argv = games, episodes, seed, prob.
// Prints one JSON line: what xq::ReplayBuffer::colourSwap() reports around setColourSwap, whether 1.5 and NaN were refused
// (std::invalid_argument), and for a batched train() with a replay ring under the default and under xq::ChessAI::setColourSwap(prob):
// TrainStats::colour_swap of the trainer's ring as the run ended, the updates done and whether every parameter came out finite.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static double train(xq::ChessAI& ai, int games, int episodes, uint64_t seed, unsigned long long* updates, int* finite) {
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setParallelGames(games);
    ai.setReplay(games * 16, games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    *updates = ai.lastTrainStats().updates;
    std::vector<double> w, b;
    ai.network()->getParameters(w, b);
    *finite = 1;
    for (double v : w) *finite = *finite && std::isfinite(v);
    for (double v : b) *finite = *finite && std::isfinite(v);
    return ai.lastTrainStats().colour_swap;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const double prob = std::atof(argv[4]);
    xq::ReplayBuffer ring(64, seed);
    const double ringBefore = ring.colourSwap();
    ring.setColourSwap(prob);
    const double ringAfter = ring.colourSwap();
    int bigRefused = 0, nanRefused = 0, aiNegRefused = 0, aiNanRefused = 0;
    try { ring.setColourSwap(1.5); } catch (const std::invalid_argument&) { bigRefused = 1; }
    try { ring.setColourSwap(std::nan("")); } catch (const std::invalid_argument&) { nanRefused = 1; }
    const double ringMirror = ring.mirror();                                 // the mirror's setting is another one
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    try { ai.setColourSwap(-0.1); } catch (const std::invalid_argument&) { aiNegRefused = 1; }
    try { ai.setColourSwap(std::nan("")); } catch (const std::invalid_argument&) { aiNanRefused = 1; }
    const double aiBefore = ai.colourSwap();
    unsigned long long u0 = 0, u1 = 0;
    int f0 = 0, f1 = 0;
    const double plain = train(ai, games, episodes, seed, &u0, &f0);
    ai.setColourSwap(prob);
    const double swapped = train(ai, games, episodes, seed, &u1, &f1);
    std::printf("{\"ring_before\": %.17g, \"ring_after\": %.17g, \"ring_mirror\": %.17g, \"big_refused\": %d, \"nan_refused\": %d, "
                "\"ai_neg_refused\": %d, \"ai_nan_refused\": %d, \"ai_before\": %.17g, \"ai_after\": %.17g, \"plain_swap\": %.17g, "
                "\"plain_updates\": %llu, \"plain_finite\": %d, \"swapped_swap\": %.17g, \"swapped_updates\": %llu, \"swapped_finite\": %d, "
                "\"stats_mirror\": %.17g}\n",
                ringBefore, ringAfter, ringMirror, bigRefused, nanRefused, aiNegRefused, aiNanRefused, aiBefore, ai.colourSwap(), plain, u0,
                f0, swapped, u1, f1, ai.lastTrainStats().mirror);
    return 0;
}
