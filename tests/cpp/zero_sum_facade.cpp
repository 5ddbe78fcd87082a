// The zero-sum target through the header-only facade (tests/test_zero_sum_facade_gpu.py): argv = games, episodes, seed.
// Prints one JSON line: what xq::DQN::zeroSum() reports around setZeroSum, whether the single-board loops of xq::ChessAI refuse it
// (std::invalid_argument), both directions of the conflict with setOpponent, and for a batched self-play train() with a replay ring with
// and without xq::ChessAI::setZeroSum(true): TrainStats::zero_sum as the run ended, the updates done, and whether the two runs, from the
// same seeds and weights, left different parameters (the flag reaches the trainer's net).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static const std::vector<int> kSizes{90 * 14, 64, 64, 90 * 90};

struct Run { bool zero_sum; unsigned long long updates; std::vector<double> w; bool finite; };

static Run train(xq::ChessAI& ai, int games, int episodes, uint64_t seed) {
    ai.setDQN(std::make_unique<xq::DQN>(kSizes, 0.01, 0.99, seed));
    ai.setParallelGames(games);
    ai.setReplay(games * 16, games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    Run r;
    r.zero_sum = ai.lastTrainStats().zero_sum;
    r.updates = ai.lastTrainStats().updates;
    std::vector<double> b;
    ai.network()->getParameters(r.w, b);
    r.finite = true;
    for (double v : r.w) r.finite = r.finite && std::isfinite(v);
    return r;
}

template <class F> static int refused(F f) {
    try { f(); } catch (const std::invalid_argument&) { return 1; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    xq::DQN net(kSizes, 0.01, 0.99, seed);
    const int before = net.zeroSum() ? 1 : 0;
    net.setZeroSum(true);
    const int after = net.zeroSum() ? 1 : 0;
    net.setOptimizer(xq::Optimizer::adam());
    net.updateTargetNetwork();
    const int kept = net.zeroSum() ? 1 : 0;
    net.setZeroSum(false);
    const int back = net.zeroSum() ? 1 : 0;

    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    const int aiBefore = ai.zeroSum() ? 1 : 0;
    // the single-board loops are the reference's: no zero-sum target there
    ai.setZeroSum(true);
    ai.setParallelGames(1);
    const int trainRefused = refused([&] { ai.train(1); });
    const int episodeRefused = refused([&] { ai.trainEpisode(); });
    const int stepRefused = refused([&] { ai.trainStep(); });
    const int selfPlayRefused = refused([&] { ai.startSelfPlay(1); });
    // zero-sum is for self-play transitions: it and an opponent refuse each other
    const int opponentRefused = refused([&] { ai.setOpponent(xq::Player::random()); });
    ai.setZeroSum(false);
    ai.setOpponent(xq::Player::random());
    const int zeroSumRefused = refused([&] { ai.setZeroSum(true); });
    const int offAllowed = 1 - refused([&] { ai.setZeroSum(false); });
    ai.clearOpponent();
    ai.setZeroSum(true);
    const int aiAfter = ai.zeroSum() ? 1 : 0;

    const Run on = train(ai, games, episodes, seed);
    ai.setZeroSum(false);
    const Run off = train(ai, games, episodes, seed);
    double diff = 0;
    for (size_t i = 0; i < on.w.size() && i < off.w.size(); ++i) diff = std::fmax(diff, std::fabs(on.w[i] - off.w[i]));
    std::printf("{\"before\": %d, \"after\": %d, \"kept\": %d, \"back\": %d, \"ai_before\": %d, \"ai_after\": %d, \"train_refused\": %d, "
                "\"episode_refused\": %d, \"step_refused\": %d, \"selfplay_refused\": %d, \"opponent_refused\": %d, \"zero_sum_refused\": %d, "
                "\"off_allowed\": %d, \"on_zero_sum\": %d, \"on_updates\": %llu, \"on_finite\": %d, \"off_zero_sum\": %d, \"off_updates\": %llu, "
                "\"off_finite\": %d, \"max_param_diff\": %.17g}\n",
                before, after, kept, back, aiBefore, aiAfter, trainRefused, episodeRefused, stepRefused, selfPlayRefused, opponentRefused,
                zeroSumRefused, offAllowed, on.zero_sum ? 1 : 0, on.updates, on.finite ? 1 : 0, off.zero_sum ? 1 : 0, off.updates,
                off.finite ? 1 : 0, diff);
    return 0;
}
