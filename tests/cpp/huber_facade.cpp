// The Huber TD loss through the header-only facade (tests/test_huber_gpu.py): argv = games, episodes, seed, kappa.
// Prints one JSON line: what xq::DQN::tdLoss() reports around xq::ChessAI::setTdLoss and setOptimizer, whether kappa = 0 was refused
// (std::invalid_argument) and tdErrorStats() throws before the first TD step, and for a batched SGD train() under huber(kappa) and the
// same one under the squared loss, from the same weights and seed: the updates done and the largest change of an output-layer weight.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static double train(xq::ChessAI& ai, const xq::TdLoss& loss, int games, int episodes, uint64_t seed, unsigned long long* updates) {
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setTdLoss(loss);
    std::vector<double> w0, b0, w1, b1;
    ai.network()->getParameters(w0, b0);
    ai.setParallelGames(games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    ai.network()->getParameters(w1, b1);
    *updates = ai.lastTrainStats().updates;
    double d = 0;
    for (size_t i = w0.size() - (size_t)sizes[1] * sizes[2]; i < w0.size(); ++i) d = std::fmax(d, std::fabs(w1[i] - w0[i]));
    return d;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const double kappa = std::strtod(argv[4], nullptr);
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    int statsRefusedBeforeStep = 0, zeroRefused = 0;
    ai.setTdLoss(xq::TdLoss::squared());
    const int before = ai.network()->tdLoss().kind;
    try {
        (void)ai.network()->tdErrorStats();
    } catch (const std::exception&) {
        statsRefusedBeforeStep = 1;
    }
    try {
        ai.setTdLoss(xq::TdLoss::huber(0.0));
    } catch (const std::invalid_argument&) {
        zeroRefused = 1;
    }
    ai.setTdLoss(xq::TdLoss::huber(kappa));
    const xq::TdLoss set = ai.network()->tdLoss();
    ai.setOptimizer(xq::Optimizer::adam());
    ai.setGradClip(1.0);
    ai.setTargetTau(0.5);
    const xq::TdLoss after = ai.network()->tdLoss();
    unsigned long long uh = 0, us = 0;
    const double dh = train(ai, xq::TdLoss::huber(kappa), games, episodes, seed, &uh);
    const double ds = train(ai, xq::TdLoss::squared(), games, episodes, seed, &us);
    std::printf("{\"before\": %d, \"set_kind\": %d, \"set_kappa\": %.17g, \"after_kind\": %d, \"after_kappa\": %.17g, \"zero_refused\": %d, "
                "\"stats_refused_before_step\": %d, \"huber_updates\": %llu, \"huber_max_dw\": %.9g, \"squared_updates\": %llu, "
                "\"squared_max_dw\": %.9g}\n",
                before, set.kind, set.kappa, after.kind, after.kappa, zeroRefused, statsRefusedBeforeStep, uh, dh, us, ds);
    return 0;
}
