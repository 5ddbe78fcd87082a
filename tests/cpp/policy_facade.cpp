// The exploration policy through the header-only facade (tests/test_boltzmann_facade_gpu.py): argv = games, episodes, seed, a model file to write.
// Prints one JSON line: what xq::ChessAI::policy() / epsilon() report around their setters, which values the setters refuse
// (std::invalid_argument), whether the single-board paths refuse Policy::boltzmann, and for three batched self-play train() runs from the
// same seeds and weights — greedy at the default epsilon, Boltzmann at epsilon 0 and greedy at epsilon 0 — what TrainStats reports as the
// run ended (policy, temperature, epsilon, the epsilon plies played) and whether the runs left different parameters.  Also
// xq::Arena::setTemperature: round trip, survival of reset(), refusals; and ChessAI::evaluateAgainst's temperature pair: against uniform-random
// play a temperature on the opponent is ignored and one on this agent's network moves the games, which tells the two arguments apart.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static const std::vector<int> kSizes{90 * 14, 64, 64, 90 * 90};

struct Run { xq::ChessAI::TrainStats st; std::vector<double> w; bool finite; };

static Run train(xq::ChessAI& ai, int games, int episodes, uint64_t seed) {
    ai.setDQN(std::make_unique<xq::DQN>(kSizes, 0.01, 0.99, seed));
    ai.setParallelGames(games);
    ai.setReplay(games * 16, games);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(episodes);
    Run r;
    r.st = ai.lastTrainStats();
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

static double maxDiff(const Run& a, const Run& b) {
    double d = 0;
    for (size_t i = 0; i < a.w.size() && i < b.w.size(); ++i) d = std::fmax(d, std::fabs(a.w[i] - b.w[i]));
    return d;
}

int main(int argc, char** argv) {
    if (argc < 5) return 2;
    const int games = std::atoi(argv[1]), episodes = std::atoi(argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();

    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    const int greedyBefore = ai.policy().kind == XQ_POLICY_GREEDY && ai.epsilon() == 0.1 ? 1 : 0;
    int setterRefusals = 0;
    for (double t : {0.0, -1.0, 1e-4, 1e4, nan, inf}) setterRefusals += refused([&] { ai.setPolicy(xq::Policy::boltzmann(t)); });
    for (double e : {-0.1, 1.1, nan}) setterRefusals += refused([&] { ai.setEpsilon(e); });
    xq::Policy odd; odd.kind = 7;
    setterRefusals += refused([&] { ai.setPolicy(odd); });
    const int unchanged = ai.policy().kind == XQ_POLICY_GREEDY && ai.epsilon() == 0.1 ? 1 : 0;

    // the single-board paths keep the reference's selectAction
    ai.setPolicy(xq::Policy::boltzmann(0.5));
    const int kept = ai.policy().kind == XQ_POLICY_BOLTZMANN && ai.policy().temperature == 0.5 ? 1 : 0;
    ai.initializeDQN();
    ai.setParallelGames(1);
    const int trainRefused = refused([&] { ai.train(1); });
    const int episodeRefused = refused([&] { ai.trainEpisode(); });
    const int stepRefused = refused([&] { ai.trainStep(); });
    const int selfPlayRefused = refused([&] { ai.startSelfPlay(1); });
    const int moveRefused = refused([&] { ai.getAIMove(xq::PieceColor::Red); });
    ai.setPolicy(xq::Policy::greedy());
    const int moveAllowed = 1 - refused([&] { ai.getAIMove(xq::PieceColor::Red); });

    const Run base = train(ai, games, episodes, seed);                  // greedy, epsilon 0.1
    ai.setPolicy(xq::Policy::boltzmann(0.5));
    ai.setEpsilon(0.0);
    const Run soft = train(ai, games, episodes, seed);                  // Boltzmann, epsilon 0
    ai.setPolicy(xq::Policy::greedy());
    const Run hard = train(ai, games, episodes, seed);                  // greedy, epsilon 0

    xq::Arena arena(4, seed, 0, 2);
    const auto t0 = arena.temperature();
    arena.setTemperature(0.5, 0.0);
    arena.reset(2);
    const auto t1 = arena.temperature();
    int arenaRefusals = 0;
    for (double t : {-1.0, 1e-4, 1e4, nan, inf}) {
        try { arena.setTemperature(t, 0.0); } catch (const std::exception&) { ++arenaRefusals; }
        try { arena.setTemperature(0.0, t); } catch (const std::exception&) { ++arenaRefusals; }
    }
    const auto t2 = arena.temperature();

    // evaluateAgainst: (file | "random", pairs, seed, opening, epsSelf, epsOpponent, tempSelf, tempOpponent) and (depth, ..., tempSelf)
    auto same = [](const xq::ArenaSummary& a, const xq::ArenaSummary& b) {
        bool eq = a.wins == b.wins && a.draws == b.draws && a.losses == b.losses;
        for (int c = 0; c < 5; ++c) eq = eq && a.causes[c] == b.causes[c];
        return eq ? 1 : 0;
    };
    const xq::ArenaSummary plain = ai.evaluateAgainst("random", 64, seed, 4);
    const int oppTempIgnored = same(plain, ai.evaluateAgainst("random", 64, seed, 4, 0.0, 0.0, 0.0, 1.0));
    const int selfTempMoves = 1 - same(plain, ai.evaluateAgainst("random", 64, seed, 4, 0.0, 0.0, 1.0, 0.0));
    ai.saveModel(argv[4]);
    const xq::ArenaSummary twins = ai.evaluateAgainst(argv[4], 64, seed, 0);             // one net against itself, greedy, no opening
    const xq::ArenaSummary warm = ai.evaluateAgainst(argv[4], 64, seed, 0, 0.0, 0.0, 1.0, 1.0);
    const int fileTempMoves = 1 - same(twins, warm);
    // the search overload has one temperature, this agent's (a young net loses every game to the search either way: the summary cannot
    // show it, the refusal of a value outside the range can)
    (void)ai.evaluateAgainst(1, 8, seed, 4, 0.0, 0.0, 1.0);
    int searchTempRefused = 0;
    try { ai.evaluateAgainst(1, 8, seed, 4, 0.0, 0.0, 5000.0); } catch (const std::exception&) { searchTempRefused = 1; }
    int evalRefused = 0;                                                // a temperature outside [1e-3, 1e3] reaches xq_arena_set_temperature
    try { ai.evaluateAgainst("random", 4, seed, 4, 0.0, 0.0, 5000.0, 0.0); } catch (const std::exception&) { evalRefused = 1; }

    auto kind = [](const Run& r) { return r.st.policy.kind; };
    std::printf("{\"greedy_before\": %d, \"setter_refusals\": %d, \"unchanged\": %d, \"kept\": %d, \"train_refused\": %d, \"episode_refused\": %d, "
                "\"step_refused\": %d, \"selfplay_refused\": %d, \"move_refused\": %d, \"move_allowed\": %d, "
                "\"base_kind\": %d, \"base_eps\": %.9g, \"base_explored\": %llu, \"base_steps\": %llu, \"base_finite\": %d, "
                "\"soft_kind\": %d, \"soft_temp\": %.9g, \"soft_eps\": %.9g, \"soft_explored\": %llu, \"soft_updates\": %llu, \"soft_finite\": %d, "
                "\"hard_kind\": %d, \"hard_eps\": %.9g, \"hard_explored\": %llu, \"hard_finite\": %d, "
                "\"soft_vs_hard\": %.17g, \"base_vs_hard\": %.17g, "
                "\"arena_t0\": [%.9g, %.9g], \"arena_t1\": [%.9g, %.9g], \"arena_t2\": [%.9g, %.9g], \"arena_refusals\": %d, "
                "\"opp_temp_ignored\": %d, \"self_temp_moves\": %d, \"file_temp_moves\": %d, \"search_temp_refused\": %d, \"eval_refused\": %d}\n",
                greedyBefore, setterRefusals, unchanged, kept, trainRefused, episodeRefused, stepRefused, selfPlayRefused, moveRefused, moveAllowed,
                kind(base), base.st.epsilon, (unsigned long long)base.st.exploredPlies, (unsigned long long)base.st.envSteps, base.finite ? 1 : 0,
                kind(soft), soft.st.policy.temperature, soft.st.epsilon, (unsigned long long)soft.st.exploredPlies,
                (unsigned long long)soft.st.updates, soft.finite ? 1 : 0,
                kind(hard), hard.st.epsilon, (unsigned long long)hard.st.exploredPlies, hard.finite ? 1 : 0,
                maxDiff(soft, hard), maxDiff(base, hard), t0.first, t0.second, t1.first, t1.second, t2.first, t2.second, arenaRefusals,
                oppTempIgnored, selfTempMoves, fileTempMoves, searchTempRefused, evalRefused);
    return 0;
}
