// xq_arena.hip — head-to-head evaluation: player A against player B over P pairs of games, all 2P games on one device;
// and xq::CheckedPlayer, "someone who moves on an env", for the arena's two sides and the trainer's opponent (xq_trainer.hip): make_player
// holds the validation of an xq_arena_player, borrowed_forward the one way a lent network is run.
//
// Per ply: the Q rows of each half of the games through the network of the player that moves there (borrowed_forward, on that network's
// stream, ordered by events) or that half's search picks (search_kernel, xq_search.hip, on the arena's stream), then one
// env_kernel<MODE_ARENA> launch (xq_env.hip) that plays the ply, freezes the games it ends and writes their records.
#include "xq_internal.h"

#include <cmath>
#include <vector>

using namespace xq;

struct xq_arena {
    int pairs = 0;
    int opening = 8;
    int ply = 0;                            // plies played since the reset (every live game has played exactly this many)
    xq_env* env = nullptr;                  // 2 * pairs games on the arena's stream
    xq::DevBuf<float> q;                    // [2 pairs][96] Q rows of the ply
    xq::DevBuf<xq_arena_game> rec;          // [2 pairs]
    xq::DevBuf<int> live;                   // device counter of live games
    xq::PinnedBuf<int> live_host;
    xq::DevBuf<xq_step_result> results;     // [2 pairs] the last ply's step results
    xq::DevBuf<int16_t> pick;               // [2 pairs] the search players' move indices of the ply (xq_search.hip)
    xq::DevBuf<uint32_t> view;              // [2 pairs][12] the boards as a mover-view net player reads them (allocated with the first one)
    xq::Event ev_env, ev_q[2], ev_view[2];  // ev_view: behind the staging of a half's view boards
    double temp[2] = {0.0, 0.0};            // Boltzmann temperature of A and B (xq_arena_set_temperature; 0 = greedy), kept over a reset
};

namespace xq {

int make_player(const xq_arena_player* in, const char* who, CheckedPlayer* out) {
    *out = CheckedPlayer();
    if (!in || in->kind == XQ_PLAYER_RANDOM) return XQ_OK;
    const xq_arena_player& x = *in;
    if (x.kind != XQ_PLAYER_NET && x.kind != XQ_PLAYER_SEARCH) return fail(XQ_ERR_INVALID_ARGUMENT, "%s has an unknown kind %d", who, x.kind);
    if (!(x.eps >= 0.0 && x.eps <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "%s epsilon must be in [0, 1]", who);
    out->kind = x.kind;
    out->eps_u32 = eps_to_u32(x.eps);
    if (x.kind == XQ_PLAYER_SEARCH) {
        if (x.depth < 1 || x.depth > 3) return fail(XQ_ERR_INVALID_ARGUMENT, "%s search depth must be 1, 2 or 3 (got %d)", who, x.depth);
        out->depth = x.depth;
        return XQ_OK;
    }
    if (!x.dqn) return fail(XQ_ERR_INVALID_ARGUMENT, "%s is a network player without a network", who);
    int nin = 0, nout = 0;
    dqn_shape(x.dqn, &nin, &nout);
    if (nin != kStateSize || nout < 90)
        return fail(XQ_ERR_INVALID_ARGUMENT, "%s needs layer_sizes[0] == 1260 and >= 90 outputs (got %d -> %d)", who, nin, nout);
    out->net = x.dqn;
    out->n_out = std::min(nout, 96);
    out->view = dqn_view(x.dqn) == XQ_VIEW_MOVER ? 1 : 0;
    return XQ_OK;
}

int borrowed_forward(xq_dqn* d, const uint32_t* boards_dev, int n, int n_out, float* q_rows_dev, hipStream_t s, hipEvent_t ev_env,
                     hipEvent_t ev_q) {
    hipStream_t ds = dqn_stream(d);
    if (ds != s) XQ_HIP(hipStreamWaitEvent(ds, ev_env, 0));
    {
        ProfilerOff off(dqn_profiler(d));    // not the handle's work
        XQ_TRY(xq_dqn_forward_boards_dev(d, XQ_NET_ONLINE, boards_dev, n, n_out, q_rows_dev, 96));
    }
    if (ds != s) {
        XQ_HIP(hipEventRecord(ev_q, ds));
        XQ_HIP(hipStreamWaitEvent(s, ev_q, 0));
    }
    return XQ_OK;
}

}  // namespace xq

namespace {

int read_live(xq_arena* a, int* n) {
    XQ_HIP(hipMemcpyAsync(a->live_host, a->live, sizeof(int), hipMemcpyDeviceToHost, a->env->stream));
    XQ_HIP(hipStreamSynchronize(a->env->stream));
    *n = *a->live_host;
    return XQ_OK;
}

// the mover of half h (0: A is Red there) at the arena's current ply: Red moves on even plies
int mover_of_half(const xq_arena* a, int h) { return ((a->ply & 1) ^ h) == 0 ? 0 : 1; }   // 0 = A, 1 = B

// one ply of players pl on the Q rows q of the halves a network player moves in (its own, or the caller's: xq_arena_ply_q_dev)
int launch_ply(xq_arena* a, const float* q, int q_stride, const CheckedPlayer pl[2]) {
    uint32_t e[2];
    int hq[2], pick_on[2], q_view[2];
    float it[2];
    for (int h = 0; h < 2; ++h) {
        const CheckedPlayer& p = pl[mover_of_half(a, h)];
        e[h] = p.eps_u32;
        hq[h] = p.kind == XQ_PLAYER_NET ? 1 : 0;
        q_view[h] = hq[h] && p.view;
        const double temp = a->temp[mover_of_half(a, h)];
        it[h] = hq[h] && temp != 0.0 ? temperature_to_inv(temp) : 0.f;
        pick_on[h] = p.kind == XQ_PLAYER_SEARCH && a->ply >= a->opening ? 1 : 0;
        if (pick_on[h])      // the searching half's picks, on the arena's stream right ahead of the ply (frozen games are skipped)
            XQ_TRY(search_pick_launch(a->env, p.depth, h * a->pairs, a->pairs, a->pairs, false, e[h], a->pick, a->env->stream));
    }
    XQ_TRY(env_arena_launch(a->env, q, q_stride, a->pairs, a->opening, e, hq, a->rec, a->live, a->results, a->pick, pick_on, q_view, it));
    a->ply += 1;
    return XQ_OK;
}

// The play loop of xq_arena_run / xq_arena_run_players: every live game has played a->ply plies, and the 200-move cap ends every game
// by ply 200; the live counter is read every kCheck plies (a read costs a stream synchronisation)
int run_players(xq_arena* a, const CheckedPlayer pl[2], int max_plies, int* plies_played) {
    int live = 0;
    XQ_TRY(read_live(a, &live));
    if (live == 0) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_run: every game has finished (xq_arena_reset starts over)");
    int played = 0;
    constexpr int kCheck = 4;
    while (a->ply < 200 && (max_plies <= 0 || played < max_plies) && live > 0) {
        if (a->ply >= a->opening) {
            XQ_HIP(hipEventRecord(a->ev_env, a->env->stream));      // once per ply, for both halves
            for (int h = 0; h < 2; ++h) {
                const CheckedPlayer& p = pl[mover_of_half(a, h)];
                const size_t off = (size_t)h * a->pairs;
                if (!p.net) continue;
                const uint32_t* boards = a->env->boards + off * kBoardWords;
                if (p.view) {        // per half and ply the side is uniform; the general kernel reads it from the games' meta anyway
                    XQ_TRY(a->view.reserve(2 * (size_t)a->pairs * kBoardWords));
                    XQ_TRY(view_boards_launch(boards, nullptr, a->env->meta + off, a->pairs, a->view + off * kBoardWords, a->env->stream));
                    boards = a->view + off * kBoardWords;
                    if (dqn_stream(p.net) != a->env->stream) XQ_HIP(hipEventRecord(a->ev_view[h], a->env->stream));
                }
                XQ_TRY(borrowed_forward(p.net, boards, a->pairs, p.n_out, a->q + off * 96, a->env->stream,
                                        p.view ? a->ev_view[h] : a->ev_env, a->ev_q[h]));
            }
        }
        XQ_TRY(launch_ply(a, a->q, 96, pl));
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
    xq_env_destroy(a->env);             // synchronises the arena's stream: the buffers below go behind it
    delete a;
    return XQ_OK;
}

static int arena_init(xq_arena* a, int n_pairs, uint64_t seed, uint32_t first_game_id, void* hip_stream) {
    a->pairs = n_pairs;
    XQ_TRY(xq_env_create(2 * n_pairs, seed, first_game_id, hip_stream, &a->env));
    const size_t n = 2 * (size_t)n_pairs;
    XQ_TRY(a->q.alloc(n * 96));
    XQ_TRY(a->rec.alloc(n));
    XQ_TRY(a->live.alloc(1));
    XQ_TRY(a->results.alloc(n));
    XQ_TRY(a->pick.alloc(n));
    XQ_TRY(a->live_host.alloc(1));
    XQ_TRY(a->ev_env.create(stream_event_flags()));
    for (auto& ev : a->ev_q) XQ_TRY(ev.create(stream_event_flags()));
    for (auto& ev : a->ev_view) XQ_TRY(ev.create(stream_event_flags()));
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
    return xq_arena_ply_q_dev_view(a, q_dev, q_stride, eps_a, eps_b, 0, 0);
}

int xq_arena_ply_q_dev_view(xq_arena* a, const float* q_dev, int q_stride, double eps_a, double eps_b, int view_a, int view_b) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    if ((view_a != 0 && view_a != 1) || (view_b != 0 && view_b != 1)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_ply_q_dev_view: a view flag is 0 or 1");
    if (q_dev && q_stride < 90) return fail(XQ_ERR_INVALID_ARGUMENT, "q_stride must be >= 90");
    if (!(eps_a >= 0.0 && eps_a <= 1.0 && eps_b >= 0.0 && eps_b <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "epsilon must be in [0, 1]");
    int live = 0;
    XQ_TRY(read_live(a, &live));
    if (live == 0) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_ply_q_dev: every game has finished");
    CheckedPlayer pl[2];       // network players whose rows the caller computed
    pl[0].kind = pl[1].kind = q_dev ? XQ_PLAYER_NET : XQ_PLAYER_RANDOM;
    pl[0].eps_u32 = eps_to_u32(eps_a);
    pl[1].eps_u32 = eps_to_u32(eps_b);
    pl[0].view = view_a; pl[1].view = view_b;
    return launch_ply(a, q_dev, q_stride, pl);
}

int xq_arena_set_temperature(xq_arena* a, double temp_a, double temp_b) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    if (!(temp_a == 0.0 || temperature_ok(temp_a)) || !(temp_b == 0.0 || temperature_ok(temp_b)))
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_arena_set_temperature: a temperature is 0 (greedy) or in [1e-3, 1e3] as fp32");
    a->temp[0] = temp_a;
    a->temp[1] = temp_b;
    return XQ_OK;
}
int xq_arena_get_temperature(const xq_arena* a, double* temp_a, double* temp_b) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    if (temp_a) *temp_a = a->temp[0];
    if (temp_b) *temp_b = a->temp[1];
    return XQ_OK;
}

int xq_arena_run_players(xq_arena* a, const xq_arena_player* pa, const xq_arena_player* pb, int max_plies, int* plies_played) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    CheckedPlayer pl[2];
    XQ_TRY(make_player(pa, "xq_arena_run_players: player A", &pl[0]));
    XQ_TRY(make_player(pb, "xq_arena_run_players: player B", &pl[1]));
    return run_players(a, pl, max_plies, plies_played);
}

int xq_arena_run(xq_arena* a, xq_dqn* dqn_a, xq_dqn* dqn_b, double eps_a, double eps_b, int max_plies, int* plies_played) {
    if (!a) return fail(XQ_ERR_INVALID_ARGUMENT, "null arena");
    if (!(eps_a >= 0.0 && eps_a <= 1.0 && eps_b >= 0.0 && eps_b <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "epsilon must be in [0, 1]");
    const xq_arena_player in[2] = {{dqn_a ? XQ_PLAYER_NET : XQ_PLAYER_RANDOM, dqn_a, 0, eps_a},
                                   {dqn_b ? XQ_PLAYER_NET : XQ_PLAYER_RANDOM, dqn_b, 0, eps_b}};
    CheckedPlayer pl[2];
    XQ_TRY(make_player(&in[0], "xq_arena_run: player A", &pl[0]));
    XQ_TRY(make_player(&in[1], "xq_arena_run: player B", &pl[1]));
    return run_players(a, pl, max_plies, plies_played);
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
