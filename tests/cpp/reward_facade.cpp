// The reward rule through the header-only facade (tests/test_reward_gpu.py): argv = games, episodes, seed.
// Prints one JSON line: what xq::VecEnv::reward() reports around setReward, whether a zero scale, a negative cost, a zero bound and a NaN
// were refused (std::invalid_argument) by the env and by xq::ChessAI, whether the single-board loops refuse Reward::delta, and for a
// batched train() with a replay ring under the default and under xq::ChessAI::setReward(Reward::delta(..)): the rule of the trainer's
// env as the run ended (TrainStats::reward) and the updates done.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static xq::Reward train(xq::ChessAI& ai, int games, int episodes, uint64_t seed, unsigned long long* updates) {
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setParallelGames(games);
    ai.setReplay(games * 16, games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    *updates = ai.lastTrainStats().updates;
    return ai.lastTrainStats().reward;
}

template <class F> static int refused(F f) {
    try { f(); } catch (const std::invalid_argument&) { return 1; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    xq::VecEnv env(8, seed);
    const xq::Reward envBefore = env.reward();
    env.setReward(xq::Reward::delta(0.002, 0.25, inf));
    const xq::Reward envAfter = env.reward();
    int envRefused = 0, aiRefused = 0;
    const xq::Reward bad[] = {xq::Reward::delta(0.0, 0.0, 1.0), xq::Reward::delta(-1.0, 0.0, 1.0), xq::Reward::delta(1e-3, -0.5, 1.0),
                              xq::Reward::delta(1e-3, 0.0, 0.0), xq::Reward::delta(nan, 0.0, 1.0), xq::Reward::delta(1e-3, nan, 1.0),
                              xq::Reward::delta(1e-3, 0.0, nan), xq::Reward::delta(inf, 0.0, 1.0), xq::Reward::delta(1e-3, inf, 1.0)};
    const int nBad = (int)(sizeof bad / sizeof bad[0]);
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    for (const xq::Reward& r : bad) {
        envRefused += refused([&] { env.setReward(r); });
        aiRefused += refused([&] { ai.setReward(r); });
    }
    xq::Reward odd; odd.kind = 7;
    envRefused += refused([&] { env.setReward(odd); });
    aiRefused += refused([&] { ai.setReward(odd); });
    const xq::Reward envKept = env.reward();             // a refused call changes nothing
    const int aiBefore = ai.reward().kind;
    // the single-board loops are the reference's: no delta rule there, and no silent training on the other reward
    ai.setReward(xq::Reward::delta());
    ai.setParallelGames(1);
    const int trainRefused = refused([&] { ai.train(1); });
    const int episodeRefused = refused([&] { ai.trainEpisode(); });
    const int stepRefused = refused([&] { ai.trainStep(); });
    const int selfPlayRefused = refused([&] { ai.startSelfPlay(1); });
    ai.setReward(xq::Reward::evaluate());
    unsigned long long u0 = 0, u1 = 0;
    const xq::Reward plain = train(ai, games, episodes, seed, &u0);
    ai.setReward(xq::Reward::delta(0.002, 0.25, 0.75));
    const xq::Reward asked = train(ai, games, episodes, seed, &u1);
    std::printf("{\"env_before\": [%d, %.17g, %.17g, %.17g], \"env_after\": [%d, %.17g, %.17g, %d], \"env_kept\": %d, \"n_bad\": %d, "
                "\"env_refused\": %d, \"ai_refused\": %d, \"ai_before\": %d, \"ai_after\": %d, \"train_refused\": %d, \"episode_refused\": %d, "
                "\"step_refused\": %d, \"selfplay_refused\": %d, \"plain\": [%d, %.17g, %.17g, %.17g], \"plain_updates\": %llu, "
                "\"asked\": [%d, %.17g, %.17g, %.17g], \"asked_updates\": %llu}\n",
                envBefore.kind, envBefore.scale, envBefore.plyCost, envBefore.bound, envAfter.kind, envAfter.scale, envAfter.plyCost,
                std::isinf(envAfter.bound) ? 1 : 0, envKept.kind == envAfter.kind && envKept.scale == envAfter.scale ? 1 : 0, nBad + 1,
                envRefused, aiRefused, aiBefore, ai.reward().kind, trainRefused, episodeRefused, stepRefused, selfPlayRefused, plain.kind,
                plain.scale, plain.plyCost, plain.bound, u0, asked.kind, asked.scale, asked.plyCost, asked.bound, u1);
    return 0;
}
