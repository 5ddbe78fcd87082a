// examples/train_selfplay.cpp — what the reference's Worker::process() (include/mainwindow.h:140-150) does, without Qt:
// construct ChessBoard + ChessAI, train N episodes, print every gameCompleted(game, red, black), save the model.
//
//   g++ -std=c++17 -O2 examples/train_selfplay.cpp -Iinclude -Lcn_chess_ai_amd -lxqhip -Wl,-rpath,$PWD/cn_chess_ai_amd -o train_selfplay
//   ./train_selfplay 2000 model.bin [parallel_games] [options]
//
// options (all beyond the reference, which has no flags at all — SURVEY section 5 "Config / flags"):
//   --replay CAP --minibatch MB   replay ring of CAP transitions, MB per update: train() then runs the throughput schedule that
//                                 bench.py measures (xq::ChessAI::setReplay); without them the loop is on-policy like the reference
//   --hidden 256,256              hidden layer widths (default 128: ChessAI::initializeDQN, chessai.cpp:395-404)
//   --save-every N                model_after_<N>_games.bin every N episodes (default 100 = chessai.cpp:165; 0 = never)
//   --derive                      layer-0 sums of s' derived from those of s (what bench.py runs; another summation order)
//   --prefill N                   N uniform-random plies in every game before training (spreads the games over all phases)
//   --seed S                      seed of the batched games (default: time, like the reference's srand(time))
//   adam                          the batched loop's optimizer: Adam (xq::Optimizer::adam(), defaults 0.9 / 0.999 / 1e-8) instead of SGD
//   clip=<max_norm>               clip the batched loop's gradient by its global L2 norm (xq::ChessAI::setGradClip; inf = measure only)
//   mirror=<prob>                 mirror augmentation of the batched loop's minibatches: each row reflected left-right with probability
//                                 prob in [0, 1] (xq::ChessAI::setMirror; 0 = off)
//   swap=<prob>                   colour-swap augmentation of the batched loop's minibatches: each row's colours exchanged (row -> 9 - row,
//                                 Red <-> Black) with probability prob in [0, 1] (xq::ChessAI::setColourSwap; 0 = off)
//   bootstrap=all|legal         target of the batched loop's TD step: the maximum over all outputs (default, chessai.cpp:126) or over the
//                                 moves the side to move can play in s' (xq::ChessAI::setTdBootstrap)
//   target=reference|zerosum      target of the batched loop's TD step in self-play: r + gamma max (default, chessai.cpp:126) or the zero-sum
//                                 (negamax) one, r - gamma max: s' has the other side to move (xq::ChessAI::setZeroSum; the sequential
//                                 loop, parallel_games = 1, refuses zerosum)
//   view=absolute|mover           how the batched loop's net reads a board: as it stands (default) or from the side to move — Black's
//                                 positions colour-swapped, outputs indexed in that view (xq::ChessAI::setView; the sequential loop,
//                                 parallel_games = 1, and getAIMove refuse mover; not together with swap=)
//   reward=evaluate|delta[:scale[:cost[:bound]]]
//                                 what the batched loop's plies write into the ring: evaluateBoard (default, chessai.cpp:115) or the
//                                 transition's change of material balance, scaled (1e-3), less a cost per ply (0), clamped to +-bound (1)
//                                 (xq::ChessAI::setReward; the sequential loop, parallel_games = 1, refuses delta)
//   policy=greedy|boltzmann:T     how the batched loop's non-epsilon plies pick: the first maximum (default, dqn.cpp:39-51) or a softmax draw
//                                 over the legal moves' values at temperature T in [1e-3, 1e3] (xq::ChessAI::setPolicy; the sequential
//                                 loop, parallel_games = 1, and getAIMove refuse boltzmann)
//   eps=E                         exploration rate of the batched loop in [0, 1] (default 0.1, chessai.cpp:106; xq::ChessAI::setEpsilon)
//   --json                        one JSON line with the loop's counters (bench.py's `facade` leg reads it)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "xq/xq.hpp"

int main(int argc, char** argv) {
    int episodes = 1000, parallel = 8192, replay = 0, minibatch = 0, save_every = 100, prefill = 0, npos = 0;
    const char* file = "model.bin";
    std::vector<int> hidden;
    bool derive = false, json = false, adam = false, legal = false, zerosum = false, mover_view = false;
    unsigned long long seed = 0;
    double clip = 0.0, mirror = 0.0, swap = 0.0;
    xq::Reward reward;
    xq::Policy policy;
    double eps = 0.1;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto next = [&]() -> const char* { if (i + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--replay") replay = std::atoi(next());
        else if (a == "--minibatch") minibatch = std::atoi(next());
        else if (a == "--save-every") save_every = std::atoi(next());
        else if (a == "--prefill") prefill = std::atoi(next());
        else if (a == "--seed") seed = std::strtoull(next(), nullptr, 0);
        else if (a == "--derive") derive = true;
        else if (a == "--json") json = true;
        else if (a == "adam") adam = true;
        else if (a.rfind("clip=", 0) == 0) {
            char* end = nullptr;
            clip = std::strtod(a.c_str() + 5, &end);
            if (end == a.c_str() + 5 || *end || !(clip >= 0.0)) { std::fprintf(stderr, "clip=: expected a max_norm >= 0 or inf, got %s\n", a.c_str() + 5); return 2; }
        }
        else if (a.rfind("bootstrap=", 0) == 0) {
            const std::string v = a.substr(10);
            if (v != "all" && v != "legal") { std::fprintf(stderr, "bootstrap=: expected all or legal, got %s\n", v.c_str()); return 2; }
            legal = v == "legal";
        }
        else if (a.rfind("target=", 0) == 0) {
            const std::string v = a.substr(7);
            if (v != "reference" && v != "zerosum") { std::fprintf(stderr, "target=: expected reference or zerosum, got %s\n", v.c_str()); return 2; }
            zerosum = v == "zerosum";
        }
        else if (a.rfind("view=", 0) == 0) {
            const std::string v = a.substr(5);
            if (v != "absolute" && v != "mover") { std::fprintf(stderr, "view=: expected absolute or mover, got %s\n", v.c_str()); return 2; }
            mover_view = v == "mover";
        }
        else if (a.rfind("reward=", 0) == 0) {
            // evaluate | delta[:scale[:cost[:bound]]]; the values are checked by ChessAI::setReward
            const std::string v = a.substr(7);
            if (v == "evaluate") reward = xq::Reward::evaluate();
            else if (v.rfind("delta", 0) == 0 && (v.size() == 5 || v[5] == ':')) {
                double p[3] = {1e-3, 0.0, 1.0};
                const char* s = v.c_str() + 5;
                for (int k = 0; k < 3 && *s == ':'; ++k) {
                    char* end = nullptr;
                    p[k] = std::strtod(s + 1, &end);
                    if (end == s + 1) { std::fprintf(stderr, "reward=: expected a number after ':', got %s\n", s + 1); return 2; }
                    s = end;
                }
                if (*s) { std::fprintf(stderr, "reward=: expected delta[:scale[:cost[:bound]]], got %s\n", v.c_str()); return 2; }
                reward = xq::Reward::delta(p[0], p[1], p[2]);
            } else { std::fprintf(stderr, "reward=: expected evaluate or delta[:scale[:cost[:bound]]], got %s\n", v.c_str()); return 2; }
        }
        else if (a.rfind("policy=", 0) == 0) {
            // greedy | boltzmann:T; the range of T is checked by ChessAI::setPolicy
            const std::string v = a.substr(7);
            if (v == "greedy") policy = xq::Policy::greedy();
            else if (v.rfind("boltzmann:", 0) == 0) {
                char* end = nullptr;
                const double t = std::strtod(v.c_str() + 10, &end);
                if (end == v.c_str() + 10 || *end) { std::fprintf(stderr, "policy=: expected a temperature after 'boltzmann:', got %s\n", v.c_str() + 10); return 2; }
                policy = xq::Policy::boltzmann(t);
            } else { std::fprintf(stderr, "policy=: expected greedy or boltzmann:T, got %s\n", v.c_str()); return 2; }
        }
        else if (a.rfind("eps=", 0) == 0) {
            char* end = nullptr;
            eps = std::strtod(a.c_str() + 4, &end);
            if (end == a.c_str() + 4 || *end || !(eps >= 0.0 && eps <= 1.0)) { std::fprintf(stderr, "eps=: expected a probability in [0, 1], got %s\n", a.c_str() + 4); return 2; }
        }
        else if (a.rfind("mirror=", 0) == 0) {
            char* end = nullptr;
            mirror = std::strtod(a.c_str() + 7, &end);
            if (end == a.c_str() + 7 || *end || !(mirror >= 0.0 && mirror <= 1.0)) { std::fprintf(stderr, "mirror=: expected a probability in [0, 1], got %s\n", a.c_str() + 7); return 2; }
        }
        else if (a.rfind("swap=", 0) == 0) {
            char* end = nullptr;
            swap = std::strtod(a.c_str() + 5, &end);
            if (end == a.c_str() + 5 || *end || !(swap >= 0.0 && swap <= 1.0)) { std::fprintf(stderr, "swap=: expected a probability in [0, 1], got %s\n", a.c_str() + 5); return 2; }
        }
        else if (a == "--hidden") {
            for (const char* p = next(); *p;) { hidden.push_back(std::atoi(p)); while (*p && *p != ',') ++p; if (*p == ',') ++p; }
        } else if (a.rfind("--", 0) == 0) { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
        else if (npos == 0) { episodes = std::atoi(argv[i]); ++npos; }
        else if (npos == 1) { file = argv[i]; ++npos; }
        else if (npos == 2) { parallel = std::atoi(argv[i]); ++npos; }
    }
    try {
        xq::ChessBoard board;                       // mainwindow.h:130-137: the caller owns the board
        xq::ChessAI ai(&board);
        ai.setParallelGames(parallel);              // 1 = the reference's sequential loop
        if (!hidden.empty()) {
            std::vector<int> sizes{90 * 14};
            for (int h : hidden) sizes.push_back(h);
            sizes.push_back(90 * 90);
            ai.setDQN(std::make_unique<xq::DQN>(sizes));
        }
        if (adam) ai.setOptimizer(xq::Optimizer::adam());
        if (clip != 0.0) ai.setGradClip(clip);
        if (mirror != 0.0) ai.setMirror(mirror);
        if (swap != 0.0) ai.setColourSwap(swap);
        if (legal) ai.setTdBootstrap(xq::TdBootstrap::legal());
        if (zerosum) ai.setZeroSum(true);
        if (mover_view) ai.setView(xq::View::Mover);          // (after --hidden's setDQN: the view is the network's too)
        ai.setReward(reward);
        ai.setPolicy(policy);
        ai.setEpsilon(eps);
        if (replay > 0) ai.setReplay(replay, minibatch);
        ai.setSaveInterval(save_every);
        ai.setLayer0Derive(derive);
        ai.setPrefillRandomPlies(prefill);
        if (seed) ai.setBatchSeed(seed);
        int red = 0, black = 0, games = 0;
        ai.gameCompleted = [&](int game, int redScore, int blackScore) {
            ++games; red += redScore; black += blackScore;
            if (!json && game % 500 == 0) std::printf("Game %d completed. Red score: %d Black score: %d\n", game, redScore, blackScore);
        };
        ai.trainingFinished = [&] { ai.saveModel(file); };      // Worker::onTrainingFinished, mainwindow.h:159-167
        const auto t0 = std::chrono::steady_clock::now();
        ai.train(episodes);
        const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const xq::ChessAI::TrainStats st = ai.lastTrainStats();
        if (json) {
            std::printf("{\"entry_point\": \"xq::ChessAI::train(%d)\", \"parallel_games\": %d, \"replay_capacity\": %d, \"minibatch\": %d, "
                        "\"episodes_reported\": %d, \"episodes_finished\": %llu, \"env_steps\": %llu, \"updates\": %llu, "
                        "\"loop_seconds\": %.6f, \"train_call_seconds\": %.6f, \"env_steps_per_s\": %.1f, \"updates_per_s\": %.1f, "
                        "\"screened_steps\": %llu, \"guard_fallbacks\": %llu, \"candidate_groups_per_sample\": %.3f, \"whole_groups_per_sample\": %.3f, "
                        "\"policy\": \"%s\", \"temperature\": %.9g, \"epsilon\": %.9g, \"explored_plies\": %llu}\n",
                        episodes, parallel, replay, minibatch, games, (unsigned long long)st.episodes, (unsigned long long)st.envSteps,
                        (unsigned long long)st.updates, st.seconds, s, st.seconds > 0 ? st.envSteps / st.seconds : 0.0,
                        st.seconds > 0 ? st.updates / st.seconds : 0.0, (unsigned long long)st.screenedSteps, (unsigned long long)st.guardFallbacks, st.candidateGroupsPerSample, st.wholeGroupsPerSample,
                        st.policy.kind == XQ_POLICY_BOLTZMANN ? "boltzmann" : "greedy", st.policy.temperature, st.epsilon, (unsigned long long)st.exploredPlies);
            return 0;
        }
        std::printf("%d episodes in %.2f s (%.0f episodes/s), mean captured material red %.1f black %.1f, model -> %s\n", games, s,
                    games / s, games ? (double)red / games : 0.0, games ? (double)black / games : 0.0, file);
        if (st.zero_sum) std::printf("target: zero-sum (y = r - gamma max)\n");
        if (st.view == xq::View::Mover) std::printf("view: mover (Black's positions colour-swapped)\n");
        if (st.seconds > 0)
            std::printf("batched loop: %llu plies + %llu updates in %.3f s = %.2f M env steps/s + %.0f updates/s\n",
                        (unsigned long long)st.envSteps, (unsigned long long)st.updates, st.seconds, st.envSteps / st.seconds / 1e6,
                        st.updates / st.seconds);
        if (st.policy.kind == XQ_POLICY_BOLTZMANN) std::printf("policy: boltzmann, temperature %g\n", st.policy.temperature);
        if (mover_view || policy.kind != XQ_POLICY_GREEDY) return 0;   // getAIMove reads the absolute board and picks as the reference: it refuses both
        const auto mv = ai.getAIMove(xq::PieceColor::Red);       // the GUI's "AI move" path, chessai.cpp:29-83
        std::printf("AI move for Red from the final position of the caller's board: (%d,%d) -> (%d,%d)\n", mv.first.first,
                    mv.first.second, mv.second.first, mv.second.second);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
