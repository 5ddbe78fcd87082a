// Gradient clipping through the header-only facade (tests/test_clip_gpu.py): argv = games, episodes, seed, max_norm.
// Prints one JSON line: what xq::DQN::gradClip() reports around xq::ChessAI::setGradClip and setOptimizer, whether a negative max_norm
// was refused (std::invalid_argument) and gradClipStats() throws while clipping is off, and for a batched SGD train() clipped at
// max_norm and the same one with max_norm = +inf, from the same weights and seed: the updates done and the largest change of a weight.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static double train(xq::ChessAI& ai, double maxNorm, int games, int episodes, uint64_t seed, unsigned long long* updates) {
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setGradClip(maxNorm);
    std::vector<double> w0, b0, w1, b1;
    ai.network()->getParameters(w0, b0);
    ai.setParallelGames(games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    ai.network()->getParameters(w1, b1);
    *updates = ai.lastTrainStats().updates;
    double d = 0;
    for (size_t i = 0; i < w0.size(); ++i) d = std::fmax(d, std::fabs(w1[i] - w0[i]));
    return d;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const double maxNorm = std::strtod(argv[4], nullptr);
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    int statsRefusedWhileOff = 0, negativeRefused = 0;
    const double before = ai.network() ? ai.network()->gradClip() : 0.0;
    ai.setGradClip(0.0);
    try {
        (void)ai.network()->gradClipStats();
    } catch (const std::exception&) {
        statsRefusedWhileOff = 1;
    }
    try {
        ai.setGradClip(-1.0);
    } catch (const std::invalid_argument&) {
        negativeRefused = 1;
    }
    ai.setGradClip(maxNorm);
    const double set = ai.network()->gradClip();
    ai.setOptimizer(xq::Optimizer::adam());
    const double afterOptimizer = ai.network()->gradClip();
    const xq::DQN::GradClipStats s = ai.network()->gradClipStats();
    unsigned long long uc = 0, ui = 0;
    const double dc = train(ai, maxNorm, games, episodes, seed, &uc);
    const double di = train(ai, std::numeric_limits<double>::infinity(), games, episodes, seed, &ui);
    std::printf("{\"before\": %.17g, \"set\": %.17g, \"after_optimizer\": %.17g, \"negative_refused\": %d, \"stats_refused_while_off\": %d, "
                "\"fresh_applies\": %llu, \"clip_updates\": %llu, \"clip_max_dw\": %.9g, \"inf_updates\": %llu, \"inf_max_dw\": %.9g}\n",
                before, set, afterOptimizer, negativeRefused, statsRefusedWhileOff, (unsigned long long)s.applies, uc, dc, ui, di);
    return 0;
}
