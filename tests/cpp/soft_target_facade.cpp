// Soft target update through the header-only facade (tests/test_soft_target_gpu.py): argv = seed.
// Prints one JSON line: what xq::DQN::targetTau() reports around xq::ChessAI::setTargetTau, setOptimizer and setGradClip, whether a tau
// outside [0, 1] was refused (std::invalid_argument), and the largest difference between the target net after
// xq::DQN::updateTargetNetwork(0.5) and after xq_dqn_soft_update_target(handle, 0.5) on a second network with the same parameters (0: the
// facade is the C ABI call), how far that update moved the target, and whether updateTargetNetwork(1.0) left the online net's values.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "xq/xq.hpp"

static void fill(std::vector<double>& w, std::vector<double>& b, uint64_t seed) {
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 1;
    auto next = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (double)(x >> 11) / 9007199254740992.0 * 0.1 - 0.05; };
    for (auto& v : w) v = (double)(float)next();
    for (auto& v : b) v = (double)(float)next();
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const uint64_t seed = std::strtoull(argv[1], nullptr, 10);
    xq::ChessBoard board;
    xq::ChessAI ai(&board);
    ai.setTargetTau(0.0);
    const double before = ai.network()->targetTau();
    int refused = 0;
    for (double bad : {-0.1, 1.5, std::nan("")}) {
        try {
            ai.setTargetTau(bad);
        } catch (const std::invalid_argument&) {
            ++refused;
        }
    }
    ai.setTargetTau(0.01);
    const double set = ai.network()->targetTau();
    ai.setOptimizer(xq::Optimizer::adam());
    ai.setGradClip(1.0);
    const double after = ai.network()->targetTau();

    const std::vector<int> sizes{90 * 14, 128, 90 * 90};
    xq::DQN a(sizes, 0.001, 0.99, seed), c(sizes, 0.001, 0.99, seed);
    std::vector<double> w, b, wt, bt;
    a.getParameters(w, b);
    wt = w; bt = b;
    fill(wt, bt, seed);
    for (xq::DQN* d : {&a, &c}) d->setParameters(wt, bt, XQ_NET_TARGET);
    a.updateTargetNetwork(0.5);
    if (xq_dqn_soft_update_target(c.handle(), 0.5) != XQ_OK) return 3;
    std::vector<double> wa, ba, wc, bc;
    a.getParameters(wa, ba, XQ_NET_TARGET);
    c.getParameters(wc, bc, XQ_NET_TARGET);
    double diff = 0, moved = 0, off_mid = 0;
    for (size_t i = 0; i < wa.size(); ++i) {
        diff = std::fmax(diff, std::fabs(wa[i] - wc[i]));
        moved = std::fmax(moved, std::fabs(wa[i] - wt[i]));
        off_mid = std::fmax(off_mid, std::fabs(wa[i] - 0.5 * (w[i] + wt[i])));
    }
    for (size_t i = 0; i < ba.size(); ++i) diff = std::fmax(diff, std::fabs(ba[i] - bc[i]));
    a.updateTargetNetwork(1.0);
    a.getParameters(wa, ba, XQ_NET_TARGET);
    int copied = 1;
    for (size_t i = 0; i < wa.size(); ++i) copied &= wa[i] == w[i];
    for (size_t i = 0; i < ba.size(); ++i) copied &= ba[i] == b[i];
    std::printf("{\"before\": %.17g, \"set\": %.17g, \"after\": %.17g, \"refused\": %d, \"facade_vs_capi\": %.9g, \"moved\": %.9g, "
                "\"off_midpoint\": %.9g, \"tau_one_is_the_copy\": %d}\n", before, set, after, refused, diff, moved, off_mid, copied);
    return 0;
}
