// The mover view through the header-only facade (tests/test_view_facade_gpu.py): argv = games, episodes, seed.
// Prints one JSON line: what xq::DQN::view() reports around setView, whether the single-board paths of xq::ChessAI refuse the view
// (std::invalid_argument), both directions of the conflict with setColourSwap, and for a batched self-play train() with a replay ring with
// and without xq::ChessAI::setView(xq::View::Mover): TrainStats::view as the run ended, the updates done, and whether the two runs, from
// the same seeds and weights, left different parameters (the setting reaches the trainer).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static const std::vector<int> kSizes{90 * 14, 64, 64, 90 * 90};

struct Run { bool mover; unsigned long long updates; std::vector<double> w; bool finite; bool netKept; };

static Run train(xq::ChessAI& ai, int games, int episodes, uint64_t seed) {
    ai.setDQN(std::make_unique<xq::DQN>(kSizes, 0.01, 0.99, seed));
    ai.setParallelGames(games);
    ai.setReplay(games * 16, games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    Run r;
    r.mover = ai.lastTrainStats().view == xq::View::Mover;
    r.updates = ai.lastTrainStats().updates;
    r.netKept = ai.network()->view() == ai.view();          // setDQN carried the agent's view onto the new network
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
    const int before = net.view() == xq::View::Mover ? 1 : 0;
    net.setView(xq::View::Mover);
    const int after = net.view() == xq::View::Mover ? 1 : 0;
    net.setOptimizer(xq::Optimizer::adam());
    net.setZeroSum(true);
    net.updateTargetNetwork();
    const int kept = net.view() == xq::View::Mover ? 1 : 0;
    net.setView(xq::View::Absolute);
    const int back = net.view() == xq::View::Mover ? 1 : 0;

    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    const int aiBefore = ai.view() == xq::View::Mover ? 1 : 0;
    // the single-board paths read the absolute board: no mover view there
    ai.setView(xq::View::Mover);
    ai.setParallelGames(1);
    const int trainRefused = refused([&] { ai.train(1); });
    const int episodeRefused = refused([&] { ai.trainEpisode(); });
    const int stepRefused = refused([&] { ai.trainStep(); });
    const int selfPlayRefused = refused([&] { ai.startSelfPlay(1); });
    const int moveRefused = refused([&] { ai.getAIMove(xq::PieceColor::Red); });
    // the view of a swapped transition is the view of the transition: the two refuse each other
    const int swapRefused = refused([&] { ai.setColourSwap(0.5); });
    const int swapOffAllowed = 1 - refused([&] { ai.setColourSwap(0.0); });
    ai.setView(xq::View::Absolute);
    ai.setColourSwap(0.5);
    const int viewRefused = refused([&] { ai.setView(xq::View::Mover); });
    ai.setColourSwap(0.0);
    ai.setView(xq::View::Mover);
    const int aiAfter = ai.view() == xq::View::Mover ? 1 : 0;

    const Run on = train(ai, games, episodes, seed);
    ai.setView(xq::View::Absolute);
    const Run off = train(ai, games, episodes, seed);
    double diff = 0;
    for (size_t i = 0; i < on.w.size() && i < off.w.size(); ++i) diff = std::fmax(diff, std::fabs(on.w[i] - off.w[i]));
    std::printf("{\"before\": %d, \"after\": %d, \"kept\": %d, \"back\": %d, \"ai_before\": %d, \"ai_after\": %d, \"train_refused\": %d, "
                "\"episode_refused\": %d, \"step_refused\": %d, \"selfplay_refused\": %d, \"move_refused\": %d, \"swap_refused\": %d, "
                "\"swap_off_allowed\": %d, \"view_refused\": %d, \"on_mover\": %d, \"on_updates\": %llu, \"on_finite\": %d, \"on_net_kept\": %d, "
                "\"off_mover\": %d, \"off_updates\": %llu, \"off_finite\": %d, \"off_net_kept\": %d, \"max_param_diff\": %.17g}\n",
                before, after, kept, back, aiBefore, aiAfter, trainRefused, episodeRefused, stepRefused, selfPlayRefused, moveRefused,
                swapRefused, swapOffAllowed, viewRefused, on.mover ? 1 : 0, on.updates, on.finite ? 1 : 0, on.netKept ? 1 : 0,
                off.mover ? 1 : 0, off.updates, off.finite ? 1 : 0, off.netKept ? 1 : 0, diff);
    return 0;
}
