// xq_arena.hip — head-to-head evaluation: player A against player B over P pairs of games, all 2P games on one device.
//
// Per ply: the Q rows of each half of the games through the network of the player that moves there (xq_dqn_forward_boards_dev on that
// network's stream, ordered by events) or that half's search picks (search_kernel, xq_search.hip, on the arena's stream), then one
// env_kernel<MODE_ARENA> launch (xq_env.hip) that plays the ply, freezes the games it ends and writes their records.  The networks are
// borrowed: the forwards keep no layer-0 sums, touch no TD-step state and are not counted by the handle's kernel statistics.
#include "xq_internal.h"

#include <algorithm>
#include <cmath>
#include <vector>

using namespace xq;

struct xq_arena {
    int pairs = 0;
    int opening = 8;
    int ply = 0;                            // plies played since the reset (every live game has played exactly this many)
    xq_env* env = nullptr;                  // 2 * pairs games on the arena's stream
    float* q = nullptr;                     // [2 pairs][96] Q rows of the ply
    xq_arena_game* rec = nullptr;           // [2 pairs]
    int* live = nullptr;                    // device counter of live games
    int* live_host = nullptr;               // pinned
    xq_step_result* results = nullptr;      // [2 pairs] the last ply's step results
    int16_t* pick = nullptr;                // [2 pairs] the search players' move indices of the ply (xq_search.hip)
    hipEvent_t ev_env = nullptr, ev_q[2] = {nullptr, nullptr};
};

namespace {

uint32_t eps_u32(double eps) { return (uint32_t)std::min(std::max(eps, 0.0) * 4294967296.0, 4294967295.0); }

int read_live(xq_arena* a, int* n) {
    XQ_HIP(hipMemcpyAsync(a->live_host, a->live, sizeof(int), hipMemcpyDeviceToHost, a->env->stream));
    XQ_HIP(hipStreamSynchronize(a->env->stream));
    *n = *a->live_host;
    return XQ_OK;
}

// the mover of half h (0: A is Red there) at the arena's current ply: Red moves on even plies
int mover_of_half(const xq_arena* a, int h) { return ((a->ply & 1) ^ h) == 0 ? 0 : 1; }   // 0 = A, 1 = B

int launch_ply(xq_arena* a, const float* q, int q_stride, const double eps[2], const bool has_q[2], const int depth[2] = nullptr) {
    uint32_t e[2];
    int hq[2], pick_on[2];
    for (int h = 0; h < 2; ++h) {
        const int p = mover_of_half(a, h);
        e[h] = eps_u32(eps[p]);
        hq[h] = has_q[p] ? 1 : 0;
        pick_on[h] = depth && depth[p] > 0 && a->ply >= a->opening ? 1 : 0;
        if (pick_on[h])      // the searching half's picks, on the arena's stream right ahead of the ply (frozen games are skipped)
            XQ_TRY(search_pick_launch(a->env, depth[p], h * a->pairs, a->pairs, a->pairs, e[h], a->pick));
    }
    XQ_TRY(env_arena_launch(a->env, q, q_stride, a->pairs, a->opening, e, hq, a->rec, a->live, a->results, a->pick, pick_on));
    a->ply += 1;
    return XQ_OK;
}

// Q rows of half h through network d, on d's stream, behind the arena's last ply and ahead of its next
int half_forward(xq_arena* a, xq_dqn* d, int h, int n_out) {
    hipStream_t s = dqn_stream(d), as = a->env->stream;
    if (s != as) XQ_HIP(hipStreamWaitEvent(s, a->ev_env, 0));
    Profiler* prof = dqn_profiler(d);
    const bool was = prof->enabled;
    prof->enabled = false;                   // the arena's forwards are not the handle's work: they stay out of its kernel statistics
    const size_t off = (size_t)h * a->pairs;
    const int rc = xq_dqn_forward_boards_dev(d, XQ_NET_ONLINE, a->env->boards + off * kBoardWords, a->pairs, n_out, a->q + off * 96, 96);
    prof->enabled = was;
    XQ_TRY(rc);
    if (s != as) {
        XQ_HIP(hipEventRecord(a->ev_q[h], s));
        XQ_HIP(hipStreamWaitEvent(as, a->ev_q[h], 0));
    }
    return XQ_OK;
}

// one player of the arena: a network (net), the material search (depth > 0) or uniform-random play (neither)
struct Policy {
    xq_dqn* net = nullptr;
    int depth = 0;
    double eps = 0.0;
};

int check_net(xq_dqn* d, int* n_out) {
    if (!d) return XQ_OK;
    int nin = 0, nout = 0;
    dqn_shape(d, &nin, &nout);
    if (nin != kStateSize || nout < 90)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena: a player needs layer_sizes[0] == 1260 and >= 90 outputs (got %d -> %d)", nin, nout);
    *n_out = std::min(nout, 96);
    return XQ_OK;
}

// The play loop of xq_arena_run / xq_arena_run_players: every live game has played a->ply plies, and the 200-move cap ends every game
// by ply 200; the live counter is read every kCheck plies (a read costs a stream synchronisation)
int run_policies(xq_arena* a, const Policy pol[2], int max_plies, int* plies_played) {
    int out[2] = {96, 96};
    XQ_TRY(check_net(pol[0].net, &out[0]));
    XQ_TRY(check_net(pol[1].net, &out[1]));
    int live = 0;
    XQ_TRY(read_live(a, &live));
    if (live == 0) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_run: every game has finished (xq_arena_reset starts over)");
    const double eps[2] = {pol[0].eps, pol[1].eps};
    const bool has_q[2] = {pol[0].net != nullptr, pol[1].net != nullptr};
    const int depth[2] = {pol[0].depth, pol[1].depth};
    int played = 0;
    constexpr int kCheck = 4;
    while (a->ply < 200 && (max_plies <= 0 || played < max_plies) && live > 0) {
        if (a->ply >= a->opening) {
            XQ_HIP(hipEventRecord(a->ev_env, a->env->stream));
            for (int h = 0; h < 2; ++h) {
                const int p = mover_of_half(a, h);
                if (pol[p].net) XQ_TRY(half_forward(a, pol[p].net, h, out[p]));
            }
        }
        XQ_TRY(launch_ply(a, a->q, 96, eps, has_q, depth));
        played += 1;
        if (played % kCheck == 0) XQ_TRY(read_live(a, &live));
    }
    XQ_HIP(hipStreamSynchronize(a->env->stream));
    if (plies_played) *plies_played = played;
    return XQ_OK;
}

}  // namespace

extern "C" {

int xq_arena_destroy(xq_arena* a) {
    if (!a) return XQ_OK;
    if (a->env) hipStreamSynchronize(a->env->stream);
    hipFree(a->q); hipFree(a->rec); hipFree(a->live); hipFree(a->results); hipFree(a->pick);
    if (a->live_host) hipHostFree(a->live_host);
    if (a->ev_env) hipEventDestroy(a->ev_env);
    for (auto ev : a->ev_q) if (ev) hipEventDestroy(ev);
    xq_env_destroy(a->env);
    delete a;
    return XQ_OK;
}

static int arena_init(xq_arena* a, int n_pairs, uint64_t seed, uint32_t first_game_id, void* hip_stream) {
    a->pairs = n_pairs;
    XQ_TRY(xq_env_create(2 * n_pairs, seed, first_game_id, hip_stream, &a->env));
    const size_t n = 2 * (size_t)n_pairs;
    XQ_HIP(hipMalloc(&a->q, n * 96 * sizeof(float)));
    XQ_HIP(hipMalloc(&a->rec, n * sizeof(xq_arena_game)));
    XQ_HIP(hipMalloc(&a->live, sizeof(int)));
    XQ_HIP(hipMalloc(&a->results, n * sizeof(xq_step_result)));
    XQ_HIP(hipMalloc(&a->pick, n * sizeof(int16_t)));
    XQ_HIP(hipHostMalloc(reinterpret_cast<void**>(&a->live_host), sizeof(int), hipHostMallocDefault));
    XQ_HIP(hipEventCreateWithFlags(&a->ev_env, stream_event_flags()));
    for (auto& ev : a->ev_q) XQ_HIP(hipEventCreateWithFlags(&ev, stream_event_flags()));
    return xq_arena_reset(a, 8);
}

int xq_arena_create(int n_pairs, uint64_t seed, uint32_t first_game_id, void* hip_stream, xq_arena** out) {
    if (!out || n_pairs <= 0 || n_pairs > (1 << 29)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_create: n_pairs must be > 0");
    xq_arena* a = new xq_arena();
    const int rc = arena_init(a, n_pairs, seed, first_game_id, hip_stream);
    if (rc != XQ_OK) { xq_arena_destroy(a); return rc; }
    *out = a;
    return XQ_OK;
}

int xq_arena_reset(xq_arena* a, int opening_plies) {
    if (!a || opening_plies < 0 || opening_plies > 200) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_reset: opening_plies must be in [0, 200]");
    XQ_TRY(xq_env_reset(a->env));
    const int n = 2 * a->pairs;
    std::vector<xq_arena_game> rec((size_t)n);
    for (int g = 0; g < n; ++g) {
        xq_arena_game& r = rec[(size_t)g];
        memset(&r, 0, sizeof r);
        r.cause = XQ_ARENA_LIVE;
        r.winner = C_NONE;
        r.a_is_red = g < a->pairs ? 1 : 0;
    }
    *a->live_host = n;
    XQ_HIP(hipMemcpyAsync(a->rec, rec.data(), rec.size() * sizeof(xq_arena_game), hipMemcpyHostToDevice, a->env->stream));
    XQ_HIP(hipMemcpyAsync(a->live, a->live_host, sizeof(int), hipMemcpyHostToDevice, a->env->stream));
    XQ_HIP(hipStreamSynchronize(a->env->stream));      // (the host vector and the pinned word are reused right after)
    a->opening = opening_plies;
    a->ply = 0;
    return XQ_OK;
}

int xq_arena_ply_q_dev(xq_arena* a, const float* q_dev, int q_stride, double eps_a, double eps_b) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    if (q_dev && q_stride < 90) return fail(XQ_ERR_INVALID_ARGUMENT, "q_stride must be >= 90");
    if (!(eps_a >= 0.0 && eps_a <= 1.0 && eps_b >= 0.0 && eps_b <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "epsilon must be in [0, 1]");
    int live = 0;
    XQ_TRY(read_live(a, &live));
    if (live == 0) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_ply_q_dev: every game has finished");
    const double eps[2] = {eps_a, eps_b};
    const bool has_q[2] = {q_dev != nullptr, q_dev != nullptr};
    return launch_ply(a, q_dev, q_stride, eps, has_q);
}

int xq_arena_run(xq_arena* a, xq_dqn* dqn_a, xq_dqn* dqn_b, double eps_a, double eps_b, int max_plies, int* plies_played) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    if (!(eps_a >= 0.0 && eps_a <= 1.0 && eps_b >= 0.0 && eps_b <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "epsilon must be in [0, 1]");
    Policy pol[2];
    pol[0].net = dqn_a; pol[0].eps = eps_a;
    pol[1].net = dqn_b; pol[1].eps = eps_b;
    return run_policies(a, pol, max_plies, plies_played);
}

int xq_arena_run_players(xq_arena* a, const xq_arena_player* pa, const xq_arena_player* pb, int max_plies, int* plies_played) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    Policy pol[2];
    const xq_arena_player* in[2] = {pa, pb};
    for (int p = 0; p < 2; ++p) {
        const char* who = p == 0 ? "player A" : "player B";
        if (!in[p]) continue;                                       // uniform-random play
        const xq_arena_player& x = *in[p];
        if (x.kind == XQ_PLAYER_RANDOM) continue;
        if (x.kind != XQ_PLAYER_NET && x.kind != XQ_PLAYER_SEARCH)
            return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_run_players: %s has an unknown kind %d", who, x.kind);
        if (!(x.eps >= 0.0 && x.eps <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_run_players: %s epsilon must be in [0, 1]", who);
        if (x.kind == XQ_PLAYER_NET && !x.dqn) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_run_players: %s is a network player without a network", who);
        if (x.kind == XQ_PLAYER_SEARCH && (x.depth < 1 || x.depth > 3))
            return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_run_players: %s search depth must be 1, 2 or 3 (got %d)", who, x.depth);
        pol[p].eps = x.eps;
        if (x.kind == XQ_PLAYER_NET) pol[p].net = x.dqn;
        else pol[p].depth = x.depth;
    }
    return run_policies(a, pol, max_plies, plies_played);
}

int xq_arena_results(xq_arena* a, xq_arena_game* records_host) {
    if (!a || !records_host) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    const int n = 2 * a->pairs;
    XQ_HIP(hipMemcpyAsync(records_host, a->rec, (size_t)n * sizeof(xq_arena_game), hipMemcpyDeviceToHost, a->env->stream));
    std::vector<int32_t> meta((size_t)n * 4);
    XQ_TRY(xq_env_get_state(a->env, 0, n, nullptr, meta.data()));      // (synchronises the stream)
    for (int g = 0; g < n; ++g) {
        if (records_host[g].cause != XQ_ARENA_LIVE) continue;
        records_host[g].plies = (uint16_t)meta[(size_t)g * 4 + 0];
        records_host[g].red_score = (int16_t)meta[(size_t)g * 4 + 2];
        records_host[g].black_score = (int16_t)meta[(size_t)g * 4 + 3];
    }
    return XQ_OK;
}

int xq_arena_live(xq_arena* a, int* n_live) {
    if (!a || !n_live) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    return read_live(a, n_live);
}

int xq_arena_env(xq_arena* a, xq_env** env) {
    if (!a || !env) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    *env = a->env;
    return XQ_OK;
}

int xq_arena_last_step(xq_arena* a, xq_step_result* results_host) {
    if (!a || !results_host) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    XQ_HIP(hipMemcpyAsync(results_host, a->results, (size_t)2 * a->pairs * sizeof(xq_step_result), hipMemcpyDeviceToHost, a->env->stream));
    XQ_HIP(hipStreamSynchronize(a->env->stream));
    return XQ_OK;
}

}  // extern "C"
