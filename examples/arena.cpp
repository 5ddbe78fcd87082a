// examples/arena.cpp — did the network get stronger?  Player A (a reference-format model file) against player B (another model file,
// `random` for uniform-random play, or `search1` / `search2` / `search3` for the fixed material search of that depth, DESIGN.md §4
// "Search player") over PAIRS pairs of games on the GPU (xq::Arena, DESIGN.md §4 "Arena"); prints A's summary.
//
//   g++ -std=c++17 -O2 examples/arena.cpp -Iinclude -Lcn_chess_ai_amd -lxqhip -Wl,-rpath,$PWD/cn_chess_ai_amd -o arena
//   ./arena model_after_2000_games.bin model_after_100_games.bin [pairs] [options]
//   ./arena model.bin random 4096
//   ./arena model.bin search2 4096
//
// A may be `random` or a search too.  The topology of each model is read from the file itself (the layer sizes DQN::saveModel writes after the
// parameters, dqn.cpp:133-140).  options:
//   --seed S        Philox key of the games (default 1)
//   --opening K     uniform-random opening plies, shared by the two games of a pair (default 8)
//   --eps-a E, --eps-b E   exploration of each player (default 0: greedy)
//   --temp-a T, --temp-b T Boltzmann temperature of each player in [1e-3, 1e3] (default 0: greedy; model players only, DESIGN.md §4
//                   "Exploration policy")
//   --json          one JSON line instead of the text summary
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "xq/xq.hpp"

// `search1` .. `search3`: the depth of the search player, 0 for any other name
static int search_depth(const std::string& name) {
    return name.size() == 7 && name.compare(0, 6, "search") == 0 && name[6] >= '1' && name[6] <= '3' ? name[6] - '0' : 0;
}

// layer sizes of a reference-format model file: [weights f64][biases f64][count u64 BE][count x u32 BE]
static std::vector<int> model_layer_sizes(const std::string& path) {
    std::FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<unsigned char> bytes;
    unsigned char buf[1 << 16];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) bytes.insert(bytes.end(), buf, buf + n);
    std::fclose(f);
    auto be = [&](size_t at, int len) { uint64_t v = 0; for (int i = 0; i < len; ++i) v = v << 8 | bytes[at + i]; return v; };
    for (uint64_t cnt = 2; cnt <= XQ_MAX_LAYERS + 1; ++cnt) {
        const size_t tail = 8 + 4 * cnt;
        if (bytes.size() < tail || be(bytes.size() - tail, 8) != cnt) continue;
        std::vector<int> sizes;
        for (uint64_t i = 0; i < cnt; ++i) sizes.push_back((int)be(bytes.size() - tail + 8 + 4 * i, 4));
        uint64_t params = 0;
        for (size_t l = 0; l + 1 < sizes.size(); ++l) params += (uint64_t)sizes[l] * sizes[l + 1] + sizes[l + 1];
        if (params * 8 + tail == bytes.size()) return sizes;
    }
    throw std::runtime_error(path + " is not a reference-format model file");
}

static std::unique_ptr<xq::DQN> load_player(const std::string& path) {
    if (path == "random" || search_depth(path) > 0) return nullptr;
    auto d = std::make_unique<xq::DQN>(model_layer_sizes(path), 0.001, 0.99, 1);
    d->loadModel(path);
    return d;
}

static xq::Player as_player(const std::string& name, const xq::DQN* net, double eps) {
    if (net) return xq::Player::net(*net, eps);
    if (search_depth(name) > 0) return xq::Player::search(search_depth(name), eps);
    return xq::Player::random();
}

int main(int argc, char** argv) {
    std::vector<std::string> pos;
    unsigned long long seed = 1;
    int opening = 8;
    double eps_a = 0.0, eps_b = 0.0, temp_a = 0.0, temp_b = 0.0;
    bool json = false;
    for (int i = 1; i < argc; ++i) {
        const bool more = i + 1 < argc;
        if (!std::strcmp(argv[i], "--seed") && more) seed = std::strtoull(argv[++i], nullptr, 10);
        else if (!std::strcmp(argv[i], "--opening") && more) opening = std::atoi(argv[++i]);
        else if (!std::strcmp(argv[i], "--eps-a") && more) eps_a = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--eps-b") && more) eps_b = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--temp-a") && more) temp_a = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--temp-b") && more) temp_b = std::atof(argv[++i]);
        else if (!std::strcmp(argv[i], "--json")) json = true;
        else pos.push_back(argv[i]);
    }
    if (pos.size() < 2) {
        std::fprintf(stderr, "usage: %s MODEL_A|random|searchD MODEL_B|random|searchD [pairs] [--seed S] [--opening K] [--eps-a E] [--eps-b E] [--temp-a T] [--temp-b T] [--json]\n", argv[0]);
        return 2;
    }
    const int pairs = pos.size() > 2 ? std::atoi(pos[2].c_str()) : 1024;
    try {
        auto a = load_player(pos[0]);
        auto b = load_player(pos[1]);
        xq::Arena arena(pairs, seed, 0, opening);
        arena.setTemperature(temp_a, temp_b);
        const auto t0 = std::chrono::steady_clock::now();
        const int plies = arena.run(as_player(pos[0], a.get(), eps_a), as_player(pos[1], b.get(), eps_b));
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const xq::ArenaSummary s = arena.summary();
        if (json) {
            std::printf("{\"games\": %d, \"pairs\": %d, \"wins\": %d, \"draws\": %d, \"losses\": %d, \"scored_games\": %d, \"scored_pairs\": %d, "
                        "\"score\": %.9f, \"ci95\": [%.9f, %.9f], \"elo\": %.6f, \"causes\": [%d, %d, %d, %d, %d], \"plies\": %d, \"seconds\": %.6f}\n",
                        s.games, s.pairs, s.wins, s.draws, s.losses, s.scoredGames, s.scoredPairs, s.score, s.ciLow, s.ciHigh, s.elo,
                        s.causes[0], s.causes[1], s.causes[2], s.causes[3], s.causes[4], plies, sec);
        } else {
            std::printf("%s vs %s: %d games (%d pairs), %d plies in %.3f s (%.0f games/s)\n", pos[0].c_str(), pos[1].c_str(), s.games, s.pairs,
                        plies, sec, s.games / sec);
            std::printf("A: +%d =%d -%d  score %.4f  95%% [%.4f, %.4f]  Elo %+.1f\n", s.wins, s.draws, s.losses, s.score, s.ciLow, s.ciHigh, s.elo);
            std::printf("ended by: general captured %d, no legal move %d, 200-move cap %d, inside the opening %d, live %d\n",
                        s.causes[XQ_ARENA_GENERAL_CAPTURED], s.causes[XQ_ARENA_NO_LEGAL_MOVE], s.causes[XQ_ARENA_MOVE_CAP],
                        s.causes[XQ_ARENA_OPENING], s.causes[XQ_ARENA_LIVE]);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "arena: %s\n", e.what());
        return 1;
    }
    return 0;
}
