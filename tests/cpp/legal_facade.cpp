// Legal-move bootstrap through the header-only facade (tests/test_legal_gpu.py): argv = seed.
// Prints one JSON line: what xq::DQN::tdBootstrap() reports around setTdBootstrap, whether an unknown kind was refused, and one sided
// host step (xq_dqn_td_update_host_sided) on the start position for both colours under legal(): the move counts xq_dqn_last_legal
// reports, whether Q(s,a), y and every parameter came out finite, and whether the unsided step was refused meanwhile; then a short batched
// xq::ChessAI::train() under setTdBootstrap(legal()) with a replay ring and on-policy: the updates done and whether the parameters are finite.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <vector>

#include "xq/xq.hpp"

static int trainLegal(uint64_t seed, int ring, unsigned long long* updates) {
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    ai.setDQN(std::make_unique<xq::DQN>(sizes, 0.001, 0.99, seed));
    ai.setTdBootstrap(xq::TdBootstrap::legal());
    ai.setParallelGames(64);
    if (ring) ai.setReplay(64 * 16, 64);
    ai.setBatchSeed(seed);
    ai.setSaveInterval(0);
    ai.train(40);
    *updates = ai.lastTrainStats().updates;
    std::vector<double> w, b;
    ai.network()->getParameters(w, b);
    int finite = ai.network()->tdBootstrap().kind == XQ_BOOTSTRAP_LEGAL;
    for (double v : w) finite = finite && std::isfinite(v);
    for (double v : b) finite = finite && std::isfinite(v);
    return finite;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const uint64_t seed = std::strtoull(argv[1], nullptr, 10);
    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    xq::DQN dqn(sizes, 0.001, 0.99, seed);
    const int before = dqn.tdBootstrap().kind;
    dqn.setTdBootstrap(xq::TdBootstrap::legal());
    const int after = dqn.tdBootstrap().kind;
    int unknownRefused = 0, unsidedRefused = 0;
    xq::TdBootstrap bad; bad.kind = 7;
    try { dqn.setTdBootstrap(bad); } catch (const std::exception&) { unknownRefused = 1; }
    xq::ChessBoard board;                                       // the start position, twice: Red to move, Black to move
    uint8_t s[2 * 90];
    for (int i = 0; i < 90; ++i) {
        const xq::ChessPiece p = board.getPieceAt(i / 9, i % 9);
        s[i] = s[90 + i] = p.type == xq::PieceType::Empty ? (uint8_t)0 : (uint8_t)((int)p.type + (p.color == xq::PieceColor::Black ? 7 : 0));
    }
    const int32_t action[2] = {40, 49};
    const float reward[2] = {0.5f, -0.25f};
    const uint8_t done[2] = {0, 0}, side[2] = {0, 1};
    float q[2] = {0.f, 0.f}, y[2] = {0.f, 0.f};
    if (xq_dqn_td_update_host(dqn.handle(), 2, s, s, action, reward, done, XQ_TD_ONLINE_NET, XQ_BACKPROP_TEXTBOOK, 0.01, 0.5, q, y) ==
        XQ_ERR_INVALID_ARGUMENT)
        unsidedRefused = 1;
    if (xq_dqn_td_update_host_sided(dqn.handle(), 2, s, s, action, reward, done, side, XQ_TD_ONLINE_NET, XQ_BACKPROP_TEXTBOOK, 0.01, 0.5,
                                    q, y) != XQ_OK) {
        std::fprintf(stderr, "sided step: %s\n", xq_last_error());
        return 1;
    }
    int32_t moves[2] = {0, 0}, astar[2] = {0, 0};
    float zmax[2] = {0.f, 0.f};
    if (xq_dqn_last_legal(dqn.handle(), 2, moves, astar, zmax, nullptr) != XQ_OK) return 1;
    size_t nw = 0, nb = 0;
    if (xq_dqn_num_params(dqn.handle(), &nw, &nb) != XQ_OK) return 1;
    std::vector<double> w(nw), b(nb);
    if (xq_dqn_get_params(dqn.handle(), XQ_NET_ONLINE, w.data(), b.data()) != XQ_OK) return 1;
    int finite = std::isfinite(q[0]) && std::isfinite(q[1]) && std::isfinite(y[0]) && std::isfinite(y[1]);
    for (double v : w) finite = finite && std::isfinite(v);
    for (double v : b) finite = finite && std::isfinite(v);
    dqn.setTdBootstrap(xq::TdBootstrap::all());
    unsigned long long uRing = 0, uOn = 0;
    const int ringFinite = trainLegal(seed, 1, &uRing), onFinite = trainLegal(seed, 0, &uOn);
    std::printf("{\"train_ring_finite\": %d, \"train_ring_updates\": %llu, \"train_onpolicy_finite\": %d, \"train_onpolicy_updates\": %llu}\n",
                ringFinite, uRing, onFinite, uOn);
    std::printf("{\"before\": %d, \"after\": %d, \"back\": %d, \"unknown_refused\": %d, \"unsided_refused\": %d, \"moves_red\": %d, "
                "\"moves_black\": %d, \"astar_red\": %d, \"astar_black\": %d, \"y_red\": %.9g, \"zmax_red\": %.9g, \"finite\": %d}\n",
                before, after, dqn.tdBootstrap().kind, unknownRefused, unsidedRefused, moves[0], moves[1], astar[0], astar[1], y[0], zmax[0],
                finite);
    return 0;
}
