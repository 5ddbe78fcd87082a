// tools/refine_probe.hip — where qmax_refine2_kernel<256, true> (xq_refine.hip.h) spends its time, alone on the chip, on buffers of the
// bench's shape (n = 8192 samples, 8100 outputs = 254 lane groups in 16 row ranges, 256-wide last hidden layer, implicit replay slots).
// Two synthetic screening results: "one" = one candidate group per sample (the usual regime), "all" = one candidate in EVERY range
// (both of a thread's ranges reach the threshold).  For each: the maxima against a CPU dot, a digest of every output (compare two
// builds of the header by eye), the launch timed in a loop, and the DBG = 1 instantiation's s_memtime stamps at the level boundaries
// (median over the blocks; shares, not lengths: every stamp drains the wave's loads).  "p2" rows: DBG = 2, the second-largest values
// loaded beside the largest ones instead of behind them.
// Usage: refine_probe [n=8192] [rounds=5]
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
#include <random>
#include "../cn_chess_ai_amd/csrc/xq_internal.h"
#include "../cn_chess_ai_amd/csrc/xq_gemm.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_screen.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_gemm_dma.hip.h"
#include "../cn_chess_ai_amd/csrc/xq_l0.hip.h"           // SlotSrc
#include "../cn_chess_ai_amd/csrc/xq_td.hip.h"
#define XQ_REFINE_PROBE 1          // the stamp buffer and the clock of DBG = 1
#include "../cn_chess_ai_amd/csrc/xq_refine.hip.h"
using namespace xq;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

static int screen_row_host(int g, int code) { const int q = code & 15; return (g >> 2) * 128 + ((g >> 1) & 1) * 64 + 4 * (g & 1) + (code >> 4) * 32 + (q & 3) + 8 * (q >> 2); }
template <class T> static T* dev(const std::vector<T>& h) {
    T* d; CK(hipMalloc(&d, std::max<size_t>(h.size(), 1) * sizeof(T))); CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); return d;
}
template <class T> static T* devz(size_t count) { T* d; CK(hipMalloc(&d, count * sizeof(T))); CK(hipMemset(d, 0, count * sizeof(T))); return d; }
template <class T> static unsigned long long digest(const T* d, size_t count) {
    std::vector<T> h(count); CK(hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost));
    unsigned long long x = 1469598103934665603ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(h.data());
    for (size_t i = 0; i < count * sizeof(T); ++i) { x ^= p[i]; x *= 1099511628211ull; }
    return x;
}

enum { kStamps = 11 };
static const char* kLevel[kStamps - 1] = {"level 0: R, na, wm, stats, action records (behind the Philox rounds)", "first barrier",
                                          "level 1: b_out and the TD rows (drained here by the stamp only)", "         threshold, P1 of both ranges",
                                          "         P2 of the groups that reach the threshold", "         candidate lists (LDS atomics)",
                                          "         Q(s,a): eight wave sums, one tanh; barrier", "level 2: single candidate rows + biases", "         whole groups, barrier",
                                          "level 3: TD arithmetic + stores"};

struct Screened { float *R, *P1, *P2; };

int main(int argc, char** argv) {
    const int n = argc > 1 ? atoi(argv[1]) : 8192, rounds = argc > 2 ? atoi(argv[2]) : 5;
    const int K = 256, NO = 8100, G = 2 * ((NO + 63) / 64), ranges = 16, gpr = (G + ranges - 1) / ranges;
    const long long ldp = (n + 127) / 128 * 128;
    const int blocks = (n + kRefineSamples - 1) / kRefineSamples;
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> uw(-0.05f, 0.05f), ua(-1.f, 1.f), ub(-0.02f, 0.02f), ulow(-2.f, -1.f);
    std::vector<float> W((size_t)NO * K), Wo((size_t)NO * K), bias(NO), bo(NO), A((size_t)n * K), As((size_t)n * K), na(ldp, 0.f);
    for (auto& v : W) v = uw(rng);
    for (auto& v : Wo) v = uw(rng);
    for (auto& v : bias) v = ub(rng);
    for (auto& v : bo) v = ub(rng);
    for (auto& v : A) v = std::tanh(2.f * ua(rng));
    for (auto& v : As) v = std::tanh(2.f * ua(rng));
    float wmax = 0.f, bmax = 0.f;
    for (int j = 0; j < NO; ++j) { double s = 0; for (int k = 0; k < K; ++k) s += (double)W[(size_t)j * K + k] * W[(size_t)j * K + k]; wmax = std::max(wmax, (float)std::sqrt(s)); bmax = std::max(bmax, std::fabs(bias[j])); }
    for (int b = 0; b < n; ++b) { double s = 0; for (int k = 0; k < K; ++k) s += (double)A[(size_t)b * K + k] * A[(size_t)b * K + k]; na[b] = (float)s; }
    // the two screening results: P1 = 1.0 (+ a row tag in the low 5 bits) for the candidate groups, [-2, -1) elsewhere; P2 below every threshold
    auto tagged = [&](float v, int code) { uint32_t u; memcpy(&u, &v, 4); u = (u & ~31u) | (uint32_t)code; memcpy(&v, &u, 4); return v; };
    std::vector<float> P1[2], P2[2], R[2];
    for (int set = 0; set < 2; ++set) {
        P1[set].assign((size_t)G * ldp, -3.0e38f); P2[set].assign((size_t)G * ldp, -3.0e38f); R[set].assign((size_t)ranges * ldp, -3.0e38f);
        for (int b = 0; b < n; ++b) {
            const int win = (int)(rng() % G);
            for (int g = 0; g < G; ++g) {
                const int r = g / gpr, g0 = r * gpr, g1 = std::min(G, g0 + gpr);
                const bool cand = set == 0 ? g == win : g == g0 + b % (g1 - g0);
                const float v = tagged(cand ? 1.0f : ulow(rng), (int)(rng() & 31));
                P1[set][(size_t)g * ldp + b] = v; P2[set][(size_t)g * ldp + b] = v - 0.5f;
                R[set][(size_t)r * ldp + b] = std::max(R[set][(size_t)r * ldp + b], v);
            }
        }
    }
    // replay ring (implicit slots: the Philox stream of the sampler, as the trainer runs it)
    const uint32_t ring = 1u << 17;
    std::vector<int32_t> act(ring); std::vector<float> rew(ring); std::vector<uint8_t> done(ring);
    for (uint32_t i = 0; i < ring; ++i) {
        const uint32_t u = rng() % 100;
        act[i] = u < 2 ? -1 : u < 5 ? 96 + (int)(rng() % 8000) : (int)(rng() % 90);
        rew[i] = (float)((int)(rng() % 3) - 1); done[i] = rng() % 20 == 0;
    }
    float *dW = dev(W), *dWo = dev(Wo), *dbias = dev(bias), *dbo = dev(bo), *dA = dev(A), *dAs = dev(As), *dna = dev(na);
    Screened S[2];
    for (int set = 0; set < 2; ++set) { S[set].R = dev(R[set]); S[set].P1 = dev(P1[set]); S[set].P2 = dev(P2[set]); }
    std::vector<unsigned> wmh(6, 0u); memcpy(&wmh[0], &wmax, 4); memcpy(&wmh[4], &wmax, 4); memcpy(&wmh[2], &bmax, 4); memcpy(&wmh[5], &bmax, 4);
    unsigned* dwm = dev(wmh);
    float* zmax = devz<float>(n);
    unsigned long long* stats = devz<unsigned long long>((size_t)2 * blocks);
    TdFused T; memset(&T, 0, sizeof T);
    T.src.implicit = 1; T.src.call = 5; T.src.seed_lo = 1; T.src.seed_hi = 2; T.src.size = ring; T.src.start = 0; T.src.cap = ring;
    T.action_to = dev(act); T.reward = dev(rew); T.done = dev(done);
    T.a_s = dAs; T.w_out = dWo; T.b_out = dbo; T.view = dWo; T.view_ld = K; T.view_kmax = K; T.gamma = 0.99f;
    T.dtop = devz<float>((size_t)n * K); T.dsc = devz<float>(n); T.act = devz<int32_t>(n); T.qsa = devz<float>(n); T.yv = devz<float>(n); T.lossv = devz<float>(n);
    unsigned long long* dbg = devz<unsigned long long>((size_t)blocks * 16);
    CK(hipMemcpyToSymbol(HIP_SYMBOL(refine_dbg), &dbg, sizeof dbg));
    const size_t lds = refine_cand_words(G) * sizeof(uint32_t) + refine_wlist_bytes(G);
    auto launch = [&](auto kern, int set) {
        hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), lds, 0, S[set].R, ranges, gpr, S[set].P1, S[set].P2, G, n, ldp, dna, dA, K, dW, dbias, NO, dwm, 0,
                           zmax, stats, T, 1, SquaredLoss{});
    };
    const auto k0 = qmax_refine2_kernel<256, true, SquaredLoss, 0>;
    const auto k1 = qmax_refine2_kernel<256, true, SquaredLoss, 1>;
    const auto k2 = qmax_refine2_kernel<256, true, SquaredLoss, 2>;
    const auto k3 = qmax_refine2_kernel<256, true, SquaredLoss, 3>;
    for (auto k : {k0, k1, k2, k3}) CK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    printf("n %d: %d blocks, G %d, %d ranges of %d groups, dynamic LDS %zu bytes\n", n, blocks, G, ranges, gpr, lds);
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    int bad = 0;
    for (int set = 0; set < 2; ++set) {
        const char* name = set == 0 ? "one" : "all";
        // results: the maxima against a CPU dot of the candidate rows, and every output's digest for the three instantiations
        for (int v = 0; v < 4; ++v) {
            CK(hipMemset(stats, 0, (size_t)2 * blocks * 8));
            launch(v == 0 ? k0 : v == 1 ? k1 : v == 2 ? k2 : k3, set);
            CK(hipDeviceSynchronize());
            if (v == 0) {
                std::vector<float> z(n); CK(hipMemcpy(z.data(), zmax, (size_t)n * 4, hipMemcpyDeviceToHost));
                double worst = 0;
                for (int b = 0; b < n; b += 7) {
                    double best = -1e300;
                    for (int g = 0; g < G; ++g) {
                        const float p = P1[set][(size_t)g * ldp + b];
                        if (p < 0.5f) continue;
                        uint32_t u; memcpy(&u, &p, 4);
                        const int row = std::min(screen_row_host(g, (int)(u & 31)), NO - 1);
                        double s = bias[row];
                        for (int k = 0; k < K; ++k) s += (double)A[(size_t)b * K + k] * W[(size_t)row * K + k];
                        best = std::max(best, s);
                    }
                    worst = std::max(worst, std::fabs(best - z[b]));
                }
                std::vector<unsigned long long> st((size_t)2 * blocks); CK(hipMemcpy(st.data(), stats, st.size() * 8, hipMemcpyDeviceToHost));
                unsigned long long pairs = 0, whole = 0;
                for (int i = 0; i < blocks; ++i) { pairs += st[2 * i]; whole += st[2 * i + 1]; }
                printf("[%s] max |zmax - CPU| %.3g over every 7th sample; candidate pairs %llu (%.2f per sample), whole groups %llu\n", name, worst, pairs, (double)pairs / n, whole);
                if (!(worst < 2e-5)) ++bad;
            }
            printf("[%s] DBG %d digests: zmax %016llx dtop %016llx dsc %016llx act %016llx qsa %016llx y %016llx loss %016llx\n", name, v, digest(zmax, n),
                   digest(T.dtop, (size_t)n * K), digest(T.dsc, n), digest(T.act, n), digest(T.qsa, n), digest(T.yv, n), digest(T.lossv, n));
        }
        for (int r = 0; r < rounds; ++r) {
            float ms[2] = {0, 0};
            for (int v = 0; v < 2; ++v) {
                CK(hipEventRecord(e0, 0)); for (int i = 0; i < 20; ++i) launch(v == 0 ? k0 : k2, set); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
                CK(hipEventElapsedTime(&ms[v], e0, e1));
            }
            printf("[%s] round %d: %.2f us per launch (20 back to back); p2 beside p1 %.2f us\n", name, r, ms[0] * 50, ms[1] * 50);
        }
        for (int v = 0; v < 2; ++v) {
            for (int i = 0; i < 30; ++i) launch(v == 0 ? k1 : k3, set);
            CK(hipDeviceSynchronize());
            std::vector<unsigned long long> hd((size_t)blocks * 16); CK(hipMemcpy(hd.data(), dbg, hd.size() * 8, hipMemcpyDeviceToHost));
            auto med = [](std::vector<double> x) { std::sort(x.begin(), x.end()); return x[x.size() / 2]; };
            std::vector<double> cyc, ns;
            for (int b = 0; b < blocks; ++b) { cyc.push_back((double)(hd[b * 16 + kStamps - 1] - hd[b * 16])); ns.push_back((double)(hd[b * 16 + 12] - hd[b * 16 + 11]) * 10.0); }
            const double ghz = med(cyc) / med(ns);
            printf("[%s]%s stamps, median over %d blocks: block %.0f cycles = %.0f ns (%.2f GHz)\n", name, v ? " p2 beside p1:" : "", blocks, med(cyc), med(ns), ghz);
            for (int k = 0; k + 1 < kStamps; ++k) {
                std::vector<double> d;
                for (int b = 0; b < blocks; ++b) d.push_back((double)(hd[b * 16 + k + 1] - hd[b * 16 + k]));
                printf("    stamp %d -> %d  %7.0f cycles  %6.0f ns   %s\n", k, k + 1, med(d), med(d) / ghz, kLevel[k]);
            }
        }
    }
    return bad ? 1 : 0;
}
