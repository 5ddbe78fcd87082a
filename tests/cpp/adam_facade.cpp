// The optimizer through the header-only facade (tests/test_adam_gpu.py): argv = games, episodes, seed.
// Prints one JSON line: what xq::DQN::optimizer() reports after xq::ChessAI::setOptimizer, whether a beta of 1 was refused
// (std::invalid_argument), and for a batched train() under Adam and the same one under SGD, from the same weights and seed: the updates
// done and the largest change of a weight.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static double train(xq::ChessAI& ai, const xq::Optimizer& opt, int games, int episodes, uint64_t seed, unsigned long long* updates) {
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setOptimizer(opt);
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
    if (argc < 4) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    ai.setOptimizer(xq::Optimizer::adam(0.8, 0.99, 1e-6));
    uint64_t steps = 99;
    const xq::Optimizer set = ai.network()->optimizer(&steps);
    ai.setOptimizer(xq::Optimizer::adam());
    const xq::Optimizer def = ai.network()->optimizer();
    int refused = 0;
    try {
        ai.setOptimizer(xq::Optimizer::adam(1.0));
    } catch (const std::invalid_argument&) {
        refused = 1;
    }
    ai.setOptimizer(xq::Optimizer::sgd());
    const int back = ai.network()->optimizer().kind;
    unsigned long long ua = 0, us = 0;
    const double da = train(ai, xq::Optimizer::adam(), games, episodes, seed, &ua);
    const double ds = train(ai, xq::Optimizer::sgd(), games, episodes, seed, &us);
    std::printf("{\"kind\": %d, \"beta1\": %.17g, \"beta2\": %.17g, \"eps\": %.17g, \"steps\": %llu, \"default_beta1\": %.17g, \"default_beta2\": %.17g, "
                "\"default_eps\": %.17g, \"refused\": %d, \"kind_after_sgd\": %d, \"adam_updates\": %llu, \"adam_max_dw\": %.9g, \"sgd_updates\": %llu, "
                "\"sgd_max_dw\": %.9g}\n",
                set.kind, set.beta1, set.beta2, set.eps, (unsigned long long)steps, def.beta1, def.beta2, def.eps, refused, back, ua, da, us, ds);
    return 0;
}
