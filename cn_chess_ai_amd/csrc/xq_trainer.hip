// xq_trainer.hip — the ChessAI::train() loop (reference chessai.cpp:85-170) for n_games boards at once, on device.
//
// Per iteration (one ply in every game + one minibatch update):
//   collect : Q(s)[0..89] of every game (selectAction reads q[action.to] only, dqn.cpp:47) -> fused self-play
//             kernel (legal moves in LDS, epsilon-greedy select, movePiece, evaluateBoard, done, auto-reset) ->
//             transition written straight into the replay ring;
//   learn   : sample -> TD gradients (xq_dqn_td_grads) -> [caller all-reduces the gradient buffer over RCCL] -> SGD;
//   target  : updateTargetNetwork() every target_sync_interval updates (chessai.cpp:140 uses moveCount % 100).
// With an opponent (xq_trainer_set_opponent, DESIGN.md §4 "Versus training") a collect is the learner's half-ply between two of the
// opponent's: [its pick] -> env pre-move -> select chain -> env learner half-ply -> [its pick] -> env reply, all on the collect stream
// (versus_collect).  The opponent is an xq::CheckedPlayer, validated and run by the code the arena's players use (make_player,
// borrowed_forward: xq_arena.hip); a network opponent's forwards run on its own stream, ordered by events.
// No host round trip inside an iteration; everything is queued on one HIP stream — or, with cfg.overlap_collect, collect
// goes to a second stream: collect(t) and learn_grads(t) both read theta_t, learn_grads(t) samples the ring minus the
// slots collect(t) is writing, learn_apply(t) joins both before theta_{t+1} is written.  Preferred call order there:
// learn_grads, collect, learn_apply — collect then starts behind the column-max GEMM (which wants the chip to itself) and
// runs beside the gradient chain, which is a string of small latency-bound kernels.  collect-first is also accepted.
// Which ring slots an iteration samples, reads and retires is stated once, in xq_ring_window.h (plan_iteration, plan_rebuild).
#include "xq_internal.h"

struct xq_trainer {
    xq_trainer_config cfg;
    xq::Stream stream;                      // lent to env, dqn and replay
    xq_env* env = nullptr;
    xq_dqn* dqn = nullptr;
    xq_replay* replay = nullptr;
    uint64_t env_steps = 0, updates = 0;
    uint32_t eps_u32 = 0;
    // overlap_collect
    xq::Stream cstream;                     // collect stream
    // An event record costs the recording stream ~6 us (rocprofv3 trace), so the three marks below are recorded when somebody actually
    // has to wait for them (xq::LazyMark): `collects` once per iteration instead of once per ply, `params` / `grads` only in the
    // collect-first or mixed call orders, not on every iteration of the learn_grads -> collect loop
    xq::LazyMark params;                    // main: parameters of the next iteration are final (after learn_apply)
    xq::LazyMark collects;                  // cstream: the collects of this iteration are done
    int inflight = 0;                       // ring slots written by collects since the last learn_apply
    bool grads_queued = false;              // learn_grads already queued in this iteration: collect starts behind its big GEMM
    int prepaid_collects = 0;               // collects learn_grads had to run itself (empty ring), owed to the next collect() calls
    int excluded = 0;                       // ring slots the queued learn_grads left out of its minibatch (from write_pos - inflight)
    xq::LazyMark grads;                     // main: the queued learn_grads has finished reading the ring
    bool per_ready = false;                 // prioritized replay: the sum tree holds the ring as of the last learn_apply
    // n-step returns (xq_trainer_set_n_step; 1 = off).  tree: the readable range that goes with the tree of the last rebuild
    // (xq::RebuildPlan::tree), of which the newest (n_step - 1) * n_games are held
    int n_step = 1;
    xq::RingSpan tree;
    bool early_collect = false;             // collects_per_update > 1: collects start behind the previous parameter update (see collect_impl)
    uint64_t params_version = 0;            // dqn_params_version() when `params` was last recorded: anything that rewrote parameters on the
                                            // handle's stream since (set_params on a bf16 net, an apply_grads of the caller's own) lies
                                            // BEHIND that record, and the select chain must not start in front of it
    // versus training: the opponent (vs_on false = self-play), its picks / Q rows of the current phase, and the per-game outcome
    // counters from the learner's side {wins, draws, losses, ended} since xq_trainer_set_opponent
    bool vs_on = false;
    xq::CheckedPlayer vs;
    xq::DevBuf<int16_t> vs_pick;
    xq::DevBuf<float> vs_q;
    xq::DevBuf<uint4> vs_counts;
    xq::Event vs_ev_env, vs_ev_q;
    // mover view (xq_trainer_set_view): the env's boards as the net reads them, staged by view_boards_kernel on the collect's stream in
    // front of every select chain — the learner's (view_sel) and a versus net opponent's with a view of its own (view_opp)
    int view = XQ_VIEW_ABSOLUTE;
    xq::DevBuf<uint32_t> view_sel, view_opp;
};

using namespace xq;

extern "C" {

static int trainer_init(xq_trainer* t, const xq_trainer_config* cfg, void* hip_stream);

// records `params` here and now: the select chain may start behind this point as long as nothing rewrites parameters behind it
static int record_params(xq_trainer* t) {
    XQ_TRY(t->params.record());
    t->params_version = dqn_params_version(t->dqn);
    return XQ_OK;
}

static int plies_of(const xq_trainer* t) { return t->cfg.collects_per_update > 1 ? t->cfg.collects_per_update : 1; }

// The setters' refusal of a null handle and of a call inside an iteration: a queued learn_grads, also collects in flight, also collects played ahead
enum Busy { BUSY_GRADS, BUSY_COLLECTS, BUSY_PREPAID };
static int between_iterations(const xq_trainer* t, const char* fn, Busy b = BUSY_GRADS) {
    if (!t) return fail(XQ_ERR_INVALID_ARGUMENT, "null trainer");
    if (t->grads_queued || (b >= BUSY_COLLECTS && t->inflight > 0) || (b >= BUSY_PREPAID && t->prepaid_collects > 0))
        return fail(XQ_ERR_RUNTIME, "%s: call between iterations (after learn_apply)", fn);
    return XQ_OK;
}

int xq_trainer_create(const xq_trainer_config* cfg, void* hip_stream, xq_trainer** out) {
    if (!cfg || !out) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_create: null pointer");
    if (cfg->n_games <= 0 || cfg->n_sizes < 3 || cfg->n_sizes > XQ_MAX_LAYERS + 1)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_create: bad n_games / layer sizes");
    if (cfg->replay_capacity != 0 && cfg->replay_capacity < cfg->n_games)
        return fail(XQ_ERR_INVALID_ARGUMENT, "replay_capacity must be 0 (on-policy) or >= n_games");
    if (cfg->replay_capacity != 0 && cfg->minibatch <= 0) return fail(XQ_ERR_INVALID_ARGUMENT, "minibatch must be > 0");
    if (cfg->overlap_collect && cfg->replay_capacity == 0)
        return fail(XQ_ERR_INVALID_ARGUMENT, "overlap_collect needs a replay ring (on-policy learns on the ply just played)");
    int ndev = 0;
    XQ_TRY(xq_device_count(&ndev));
    if (ndev == 0) return fail(XQ_ERR_NO_DEVICE, "no HIP device: libxqhip has no CPU fallback");
    xq_trainer* t = new xq_trainer();
    const int rc = trainer_init(t, cfg, hip_stream);
    if (rc != XQ_OK) { xq_trainer_destroy(t); return rc; }  // a failed allocation must not leak the handles before it
    *out = t;
    return XQ_OK;
}

static int trainer_init(xq_trainer* t, const xq_trainer_config* cfg, void* hip_stream) {
    t->cfg = *cfg;
    XQ_TRY(t->stream.open(hip_stream));
    XQ_TRY(xq_env_create(cfg->n_games, cfg->seed, cfg->first_game_id, t->stream, &t->env));
    XQ_TRY(xq_dqn_create(cfg->layer_sizes, cfg->n_sizes, cfg->learning_rate, cfg->gamma, cfg->seed ^ 0x9E3779B97F4A7C15ull,
                         t->stream, &t->dqn));
    const int cap = cfg->replay_capacity > 0 ? cfg->replay_capacity : cfg->n_games;
    XQ_TRY(xq_replay_create(cap, cfg->seed + 0x1234567ull + cfg->first_game_id, t->stream, &t->replay));
    t->replay->caller_orders = true;         // env, ring and Q-net share t->stream; the collect stream is ordered below, by hand
    if (cfg->precision != XQ_PRECISION_F32) XQ_TRY(xq_dqn_set_precision(t->dqn, cfg->precision));
    if (cfg->prioritized) {
        if (cfg->replay_capacity == 0) return fail(XQ_ERR_INVALID_ARGUMENT, "prioritized replay needs a replay ring (replay_capacity > 0)");
        XQ_TRY(xq_replay_enable_per(t->replay, cfg->per_alpha > 0 ? cfg->per_alpha : 0.6, cfg->per_beta > 0 ? cfg->per_beta : 0.4,
                                    cfg->per_eps > 0 ? cfg->per_eps : 1e-3));
    }
    t->eps_u32 = eps_to_u32(cfg->epsilon);       // (a negative epsilon counts as 0)
    if (cfg->overlap_collect) {
        int lo = 0, hi = 0;
        XQ_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));        // lo = least urgent: collect has slack until learn_apply,
        // one ply per update: the TD step is the critical path, the select chain has slack until learn_apply => least urgent.
        // Several plies per update: the plies ARE the critical path (each waits for the move of the one before, bench --config 4:
        // 4 x 155 us alone, 375 + 314 us for the two that share the chip with the TD step) => most urgent: 1.096 -> 1.054 ms per step
        // (one ply per update with the select chain most urgent: no difference on the headline bench, -0.5 % on bench --config 5)
        const int prio = plies_of(t) > 1 ? hi : lo;
        XQ_TRY(t->cstream.open_owned(hipStreamNonBlocking, prio));
        XQ_TRY(t->params.open(t->stream));
        XQ_TRY(t->collects.open(t->cstream));
        XQ_TRY(t->grads.open(t->stream));
        XQ_TRY(record_params(t));                             // orders the first collect after the handles' initialisation
        t->early_collect = plies_of(t) > 1;
    }
    return XQ_OK;
}

int xq_trainer_destroy(xq_trainer* t) {
    if (!t) return XQ_OK;
    t->cstream.close();              // the collects touch env, Q-net and ring
    xq_env_destroy(t->env);          // (each synchronises the stream it was lent)
    xq_dqn_destroy(t->dqn);
    xq_replay_destroy(t->replay);
    t->stream.close();
    delete t;
    return XQ_OK;
}

int xq_trainer_env(xq_trainer* t, xq_env** e) { if (!t || !e) return fail(XQ_ERR_INVALID_ARGUMENT, "null"); *e = t->env; return XQ_OK; }
int xq_trainer_dqn(xq_trainer* t, xq_dqn** d) { if (!t || !d) return fail(XQ_ERR_INVALID_ARGUMENT, "null"); *d = t->dqn; return XQ_OK; }
int xq_trainer_replay(xq_trainer* t, xq_replay** r) { if (!t || !r) return fail(XQ_ERR_INVALID_ARGUMENT, "null"); *r = t->replay; return XQ_OK; }

// the handle's stream waits for every ply queued on the collect stream so far
static int wait_collects(xq_trainer* t) { return t->collects.wait(t->stream); }

// The opponent's half-ply of a versus collect (phase 0: the pre-move, 2: the reply) on stream s: its picks, then the env launch
static int versus_opponent(xq_trainer* t, int phase, hipStream_t s) {
    const CheckedPlayer& o = t->vs;
    const int16_t* pick = nullptr;
    const float* q = nullptr;
    int opp_view = 0;
    if (o.kind == XQ_PLAYER_SEARCH) {
        XQ_TRY(search_pick_launch(t->env, o.depth, 0, t->env->n, INT_MAX, true, o.eps_u32, t->vs_pick, s));
        pick = t->vs_pick;
    } else if (o.kind == XQ_PLAYER_NET) {
        // the opponent reads the boards through ITS OWN handle's view
        const uint32_t* boards = t->env->boards;
        if (dqn_view(o.net) == XQ_VIEW_MOVER) {
            XQ_TRY(t->view_opp.reserve((size_t)t->env->n * kBoardWords));
            XQ_TRY(view_boards_launch(t->env->boards, nullptr, t->env->meta, t->env->n, t->view_opp, s));
            boards = t->view_opp;
            opp_view = 1;
        }
        if (dqn_stream(o.net) != s) XQ_HIP(hipEventRecord(t->vs_ev_env, s));     // behind the env's last launch (and the view's)
        XQ_TRY(borrowed_forward(o.net, boards, t->env->n, o.n_out, t->vs_q, s, t->vs_ev_env, t->vs_ev_q));
        q = t->vs_q;
    }
    return env_versus_launch(t->env, phase, q, 96, nullptr, o.eps_u32, pick, t->vs_counts, t->replay, s, opp_view);
}

// The learner's select chain on stream s (`on`: the collect stream, if any): Q(s)[0..89] of every game, from the env's boards or, under
// the mover view, from their view in view_sel, staged on s in front of it
struct SelectQ { float* q90 = nullptr; int stride = 0; QSource qs; };
static int select_chain(xq_trainer* t, hipStream_t on, hipStream_t s, SelectQ* q) {
    const uint32_t* boards = t->env->boards;
    if (t->view == XQ_VIEW_MOVER) {
        XQ_TRY(view_boards_launch(t->env->boards, nullptr, t->env->meta, t->env->n, t->view_sel, s));
        boards = t->view_sel;
    }
    return dqn_q90_boards(t->dqn, boards, t->env->n, &q->q90, &q->stride, on, &q->qs);
}

// A versus collect on stream s: pre-move, select chain, learner half-ply, reply; one transition per game, into the ring slots from
// write_pos, which moves once the last phase is queued
static int versus_collect(xq_trainer* t, hipStream_t on, hipStream_t s) {
    SelectQ q;
    XQ_TRY(versus_opponent(t, 0, s));
    XQ_TRY(select_chain(t, on, s, &q));
    XQ_TRY(env_versus_launch(t->env, 1, q.q90, q.stride, &q.qs, t->eps_u32, nullptr, t->vs_counts, t->replay, s));
    XQ_TRY(versus_opponent(t, 2, s));
    replay_advance(t->replay, t->env->n);
    return XQ_OK;
}

static int collect_impl(xq_trainer* t) {
    hipStream_t on = nullptr;
    if (t->cstream) {
        on = t->cstream;
        // has anything rewritten parameters on the handle's stream since `params` was recorded?  (ORD_TRAINER_PARAMS off: the round-3
        // behaviour, for the test that shows the check is needed)
        const bool params_moved = (order_mask() & ORD_TRAINER_PARAMS) && dqn_params_version(t->dqn) != t->params_version;
        if (t->grads_queued && !t->early_collect) {
            // queued behind the column-max GEMM (which wants the chip to itself); that event lies behind every parameter update
            if (t->inflight == 0) XQ_HIP(hipStreamWaitEvent(on, dqn_qmax_event(t->dqn), 0));
        } else if (t->grads_queued) {
            // several plies per update: the collect chain is the long pole of the iteration (each ply waits for the move of the one
            // before) — it starts behind the previous parameter update, recorded there (learn_apply), and runs beside the whole TD step.
            // If parameters were rewritten behind that record, the event of the queued TD step (behind everything on the handle's
            // stream) takes its place.
            if (t->inflight == 0 && !t->params.stale && !params_moved) XQ_TRY(t->params.wait(on));
            else if (t->inflight == 0) XQ_HIP(hipStreamWaitEvent(on, dqn_qmax_event(t->dqn), 0));     // (no record yet: first iteration)
        } else if (t->inflight == 0) {
            if (t->params.stale || params_moved) XQ_TRY(record_params(t));
            XQ_TRY(t->params.wait(on));
        }
        // more plies than the queued learn_grads excluded from its minibatch (caller mixed the orders): these slots may be
        // among the ones it samples, so they can only be overwritten once it has read them
        if (t->grads_queued && t->inflight + t->env->n > t->excluded) XQ_TRY(t->grads.wait(on));
    }
    hipStream_t s = on ? on : t->stream;
    if (t->cfg.replay_capacity == 0) t->replay->write_pos = t->replay->size = 0;     // on-policy: the ring is exactly one batch, refilled every ply
    if (t->vs_on) {
        XQ_TRY(versus_collect(t, on, s));
    } else {
        SelectQ q;
        XQ_TRY(select_chain(t, on, s, &q));
        Profiler* p = dqn_profiler(t->dqn);
        const int h = p->begin("env_selfplay_step", s, true);       // one kernel: timed by its own start / stop events
        XQ_TRY(env_selfplay_launch(t->env, q.q90, q.stride, t->eps_u32, nullptr, t->replay, on, &q.qs, h >= 0 ? p->recs[h].a : nullptr,
                                   h >= 0 ? p->recs[h].b : nullptr));
        // algorithmic HBM bytes per game and ply: board+meta in/out (2*(48+16)), Q row 360, transition 48+48+4+4+1
        p->end(h, s, 0.0, (double)t->env->n * (2.0 * (48 + 16) + 360 + 105));
    }
    t->env_steps += (uint64_t)t->env->n;
    if (on) {
        t->inflight += t->env->n;
        t->collects.touched();
    }
    return XQ_OK;
}

int xq_trainer_collect(xq_trainer* t) {
    if (!t) return fail(XQ_ERR_INVALID_ARGUMENT, "null trainer");
    if (t->prepaid_collects > 0) { t->prepaid_collects--; return XQ_OK; }     // already played by learn_grads (empty ring)
    return collect_impl(t);
}

int xq_trainer_set_comm(xq_trainer* t, xq_comm* comm) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_comm"));
    return xq_dqn_set_comm(t->dqn, comm);
}

int xq_trainer_set_target_tau(xq_trainer* t, double tau) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_target_tau"));
    return xq_dqn_set_target_tau(t->dqn, tau);
}

// mirror augmentation lives on the ring and changes no window: the transform reads what the step read anyway
// The legal-move bootstrap on the trainer's Q-net; `legal` first makes the trainer's ring record the side to move in s' (possible only
// while the ring is empty: XQ_ERR_RUNTIME once it holds a transition, unless it tracks already).  Back to `all` the column stays written.
int xq_trainer_set_td_bootstrap(xq_trainer* t, int kind) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_td_bootstrap"));
    if (kind == XQ_BOOTSTRAP_LEGAL) XQ_TRY(xq_replay_track_next_player(t->replay));
    return xq_dqn_set_td_bootstrap(t->dqn, kind);
}

// The zero-sum (negamax) target on the trainer's Q-net.  It is for transitions whose s' has the other side to decide: a versus transition
// runs from one learner decision to the next, so it and xq_trainer_set_opponent refuse each other.  No window changes: only the sign of
// the discount and the no-move value of the legal bootstrap do
int xq_trainer_set_zero_sum(xq_trainer* t, int on) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_zero_sum"));
    if (on == 1 && t->vs_on)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_set_zero_sum: an opponent is set (xq_trainer_set_opponent): a versus transition ends "
                                             "with the learner to move again, which the zero-sum target is not for");
    return xq_dqn_set_zero_sum(t->dqn, on);
}

// The mover view on the trainer's Q-net, env and ring (DESIGN.md §4 "Mover view"): before the first collect, because the ring's two side
// columns can only be allocated while it is empty and a ring filled under one view is not a ring of the other.  The collects then stage
// view(board, side to move) in front of the select chain and the env picks through the view's square map; learn_grads stages the
// minibatch in the view (xq_dqn_td_grads_replay).  No window changes.
int xq_trainer_set_view(xq_trainer* t, int view) {
    if (!t) return fail(XQ_ERR_INVALID_ARGUMENT, "null trainer");
    if (view != XQ_VIEW_ABSOLUTE && view != XQ_VIEW_MOVER) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_set_view: unknown view %d", view);
    if (t->env_steps != 0 || t->grads_queued || t->inflight > 0 || t->prepaid_collects > 0 || t->replay->total != 0)
        return fail(XQ_ERR_RUNTIME, "xq_trainer_set_view: call before the first collect");
    if (view == XQ_VIEW_MOVER) {
        XQ_TRY(xq_replay_track_mover(t->replay));
        XQ_TRY(xq_replay_track_next_player(t->replay));
        XQ_TRY(t->view_sel.reserve((size_t)t->env->n * kBoardWords));
    }
    XQ_TRY(xq_dqn_set_view(t->dqn, view));
    XQ_TRY(xq_env_set_q_view(t->env, view == XQ_VIEW_MOVER ? 1 : 0));
    t->view = view;
    return XQ_OK;
}

// the reward rule of the trainer's env: the next collect writes it, slots already in the ring keep theirs
int xq_trainer_set_reward(xq_trainer* t, int kind, double scale, double ply_cost, double bound) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_reward"));
    return xq_env_set_reward(t->env, kind, scale, ply_cost, bound);
}

// The policy and the epsilon of the collects.  A launch carries both by value, so either may change between any two collects, with a
// collect of the overlap stream still in flight too: that one keeps what it was queued with
int xq_trainer_set_policy(xq_trainer* t, int kind, double temperature) {
    if (!t) return fail(XQ_ERR_INVALID_ARGUMENT, "null trainer");
    return xq_env_set_policy(t->env, kind, temperature);
}
int xq_trainer_set_epsilon(xq_trainer* t, double eps) {
    if (!t) return fail(XQ_ERR_INVALID_ARGUMENT, "null trainer");
    if (!(eps >= 0.0 && eps <= 1.0)) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_set_epsilon: eps must be in [0, 1]");
    t->cfg.epsilon = eps;
    t->eps_u32 = eps_to_u32(eps);
    return XQ_OK;
}
int xq_trainer_get_epsilon(const xq_trainer* t, double* eps) {
    if (!t || !eps) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    *eps = t->cfg.epsilon;
    return XQ_OK;
}

int xq_trainer_set_mirror(xq_trainer* t, double prob) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_mirror"));
    return xq_replay_set_mirror(t->replay, prob);
}

// ... and so does the colour swap (the side byte it flips is read at the slot the step reads it at anyway)
int xq_trainer_set_colour_swap(xq_trainer* t, double prob) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_colour_swap"));
    return xq_replay_set_colour_swap(t->replay, prob);
}

// Prioritized replay: rebuilds the tree for the ring as it stands and the next `plies` collects (xq::plan_rebuild): the slots they
// overwrite retired, the readable range that goes with the tree noted, its newest slots (incomplete chains) held out of this tree
static int rebuild_tree(xq_trainer* t, int plies) {
    const RebuildPlan p = plan_rebuild(ring_state(t->replay), t->cfg.n_games, plies, t->n_step);
    t->tree = p.tree;
    return replay_per_rebuild(t->replay, p.retire.first, p.retire.count, t->stream, p.hold.first, p.hold.count);
}

int xq_trainer_set_n_step(xq_trainer* t, int n_step) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_n_step", BUSY_PREPAID));
    const int plies = plies_of(t);
    if (n_step > 1 && t->cfg.replay_capacity == 0)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_set_n_step: n-step returns need a replay ring (on-policy keeps one ply)");
    if (n_step > 1 && n_step <= XQ_MAX_N_STEP && (long long)t->cfg.replay_capacity <= (long long)(n_step - 1 + plies) * t->cfg.n_games)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_set_n_step: the ring (%d) must exceed (n_step - 1 + collects_per_update) * n_games = %lld",
                    t->cfg.replay_capacity, (long long)(n_step - 1 + plies) * t->cfg.n_games);
    XQ_TRY(xq_replay_set_n_step(t->replay, n_step, t->cfg.n_games));
    t->n_step = n_step;
    // the tree of the last learn_apply was built for the previous hold: the same tree again (its retired slots are already 0), held anew
    if (t->cfg.prioritized && t->per_ready) {
        const RingSpan hold = span_held(t->tree, (long long)(n_step - 1) * t->cfg.n_games, t->replay->dev.capacity);
        XQ_TRY(replay_per_rebuild(t->replay, 0, 0, t->stream, hold.first, hold.count));
    }
    return XQ_OK;
}

int xq_trainer_set_td_net(xq_trainer* t, int td_net) {
    if (!t || (td_net != XQ_TD_ONLINE_NET && td_net != XQ_TD_TARGET_NET && td_net != XQ_TD_DOUBLE)) return fail(XQ_ERR_INVALID_ARGUMENT, "bad td_net");
    XQ_TRY(between_iterations(t, "xq_trainer_set_td_net"));
    t->cfg.td_net = td_net;
    return XQ_OK;
}

int xq_trainer_set_opponent(xq_trainer* t, const xq_arena_player* opp) {
    XQ_TRY(between_iterations(t, "xq_trainer_set_opponent", BUSY_PREPAID));
    CheckedPlayer vs;
    XQ_TRY(make_player(opp, "xq_trainer_set_opponent: the opponent", &vs));
    if (vs.net && vs.net == t->dqn) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_set_opponent: the opponent is the trainer's own network");
    int zero_sum = 0;
    XQ_TRY(xq_dqn_get_zero_sum(t->dqn, &zero_sum));
    if (opp && zero_sum)
        return fail(XQ_ERR_INVALID_ARGUMENT, "xq_trainer_set_opponent: the zero-sum target is on (xq_trainer_set_zero_sum): it is for self-play "
                                             "transitions, whose s' has the other side to move");
    // the previous collects are finished and nothing of the next one is queued: the buffers below are free
    if (t->cstream) XQ_HIP(hipStreamSynchronize(t->cstream));
    XQ_HIP(hipStreamSynchronize(t->stream));
    if (!opp) { t->vs_on = false; return XQ_OK; }
    const size_t n = (size_t)t->env->n;
    XQ_TRY(t->vs_counts.reserve(n));                 // (first call only: the env's size is fixed)
    XQ_TRY(t->vs_pick.reserve(n));
    XQ_TRY(t->vs_q.reserve(n * 96));
    XQ_TRY(t->vs_ev_env.create(stream_event_flags()));
    XQ_TRY(t->vs_ev_q.create(stream_event_flags()));
    XQ_HIP(hipMemsetAsync(t->vs_counts, 0, n * sizeof(uint4), t->stream));
    XQ_HIP(hipStreamSynchronize(t->stream));
    t->vs = vs;
    t->vs_on = true;
    return XQ_OK;
}

int xq_trainer_versus_results(xq_trainer* t, uint64_t out[4]) {
    if (!t || !out) return fail(XQ_ERR_INVALID_ARGUMENT, "null pointer");
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (!t->vs_counts) return XQ_OK;
    std::vector<uint4> c((size_t)t->env->n);
    if (t->cstream) XQ_HIP(hipStreamSynchronize(t->cstream));
    XQ_HIP(hipStreamSynchronize(t->stream));
    XQ_HIP(hipMemcpy(c.data(), t->vs_counts, c.size() * sizeof(uint4), hipMemcpyDeviceToHost));
    for (const uint4& v : c) { out[0] += v.x; out[1] += v.y; out[2] += v.z; out[3] += v.w; }
    return XQ_OK;
}

int xq_trainer_random_plies(xq_trainer* t, int n_plies) {
    if (!t || n_plies < 0) return fail(XQ_ERR_INVALID_ARGUMENT, "bad argument");
    XQ_TRY(between_iterations(t, "xq_trainer_random_plies", BUSY_COLLECTS));
    for (int i = 0; i < n_plies; ++i) XQ_TRY(env_selfplay_launch(t->env, nullptr, 0, 0u, nullptr, nullptr, t->stream));
    t->params.touched();                         // the next collect (own stream) starts behind these plies
    return XQ_OK;
}

// The minibatch of iteration t (xq::plan_iteration).  Uniform with overlap_collect: drawn from the ring minus the slots collect(t) writes.
// Prioritized: from the sum tree as of the last learn_apply — every transition collected before this iteration except the slots its
// collects overwrite (retired there), in both call orders.  Nothing older than this iteration's plies, or no tree yet (the first
// iteration): the plies come first, played here if need be, and the step learns on them.
int xq_trainer_learn_grads(xq_trainer* t) {
    if (!t) return fail(XQ_ERR_INVALID_ARGUMENT, "null trainer");
    const int batch = t->cfg.replay_capacity > 0 ? t->cfg.minibatch : 0;     // (on-policy: the ply just played, all of it)
    if (batch > 0) {
        const int plies = plies_of(t);
        const IterationPlan p = plan_iteration({ring_state(t->replay), t->cfg.n_games, plies, t->inflight, t->n_step, (bool)t->cstream,
                                                t->cfg.prioritized != 0, t->per_ready, t->tree});
        if (p.play_first) {
            for (int c = 0; c < plies; ++c) XQ_TRY(collect_impl(t));
            t->prepaid_collects = plies;
        }
        if (p.join_first && t->cstream) { XQ_TRY(wait_collects(t)); t->inflight = 0; }
        if (p.join_first && t->cfg.prioritized) {
            if (t->replay->size == 0) return fail(XQ_ERR_RUNTIME, "replay is empty");
            XQ_TRY(rebuild_tree(t, 0));
            t->per_ready = true;
        }
        t->excluded = p.excluded;
        if (p.readable.count >= 0) replay_set_readable(t->replay, p.readable.first, p.readable.count);
        if (t->cfg.prioritized) XQ_TRY(replay_per_sample(t->replay, batch, t->stream));
        else XQ_TRY(replay_sample_implicit(t->replay, batch, p.sample.first, p.sample.count));  // no sampling kernel: the consumers recompute the slots
    }
    XQ_TRY(xq_dqn_td_grads_replay(t->dqn, t->replay, batch, t->cfg.td_net, t->cfg.backprop_mode));
    t->grads.touched();
    t->grads_queued = true;
    return XQ_OK;
}

int xq_trainer_learn_apply(xq_trainer* t, int world_size) {
    if (!t || world_size < 1) return fail(XQ_ERR_INVALID_ARGUMENT, "bad argument");
    const int batch = t->cfg.replay_capacity > 0 ? t->cfg.minibatch : t->cfg.n_games;
    const double scale = t->cfg.mean_gradient ? 1.0 / ((double)batch * world_size) : 1.0;
    if (t->cstream && t->inflight > 0) XQ_TRY(wait_collects(t));   // the select chain reads theta_t
    XQ_TRY(xq_dqn_apply_grads(t->dqn, t->cfg.learning_rate, scale));
    t->updates += 1;
    if (t->cfg.target_sync_interval > 0 && t->updates % (uint64_t)t->cfg.target_sync_interval == 0)
        XQ_TRY(xq_dqn_update_target(t->dqn));
    if (t->cfg.prioritized) {
        // the tree of the next iteration: this iteration's TD-error priorities and new transitions in, the next collects' slots out
        XQ_TRY(rebuild_tree(t, plies_of(t)));
        t->per_ready = true;
    }
    t->params.touched();
    if (t->cstream && t->early_collect) XQ_TRY(record_params(t));    // the next iteration's collects start here, whatever the caller queues first
    t->inflight = 0;
    t->grads_queued = false;
    return XQ_OK;
}

int xq_trainer_step(xq_trainer* t, int n_iterations) {
    if (!t || n_iterations < 0) return fail(XQ_ERR_INVALID_ARGUMENT, "bad argument");
    const int plies = plies_of(t);
    if (plies > 1 && t->cfg.replay_capacity == 0)
        return fail(XQ_ERR_INVALID_ARGUMENT, "collects_per_update > 1 needs a replay ring (on-policy keeps one ply)");
    const int world = dqn_comm(t->dqn) ? comm_world(dqn_comm(t->dqn)) : 1;     // data-parallel when a communicator is attached
    const int fused_before = dqn_fused_apply(t->dqn);   // restored on every exit path: the caller's choice survives step()
    XQ_TRY(xq_dqn_set_fused_apply(t->dqn, 1));      // single-GPU loop: nothing reads the gradient buffer between grads and apply
    int rc = XQ_OK;
    for (int i = 0; i < n_iterations && rc == XQ_OK; ++i) {
        if (t->cstream) rc = xq_trainer_learn_grads(t);         // overlapped: the collects start behind its big GEMM
        for (int c = 0; c < plies && rc == XQ_OK; ++c) rc = xq_trainer_collect(t);
        if (!t->cstream && rc == XQ_OK) rc = xq_trainer_learn_grads(t);
        if (rc == XQ_OK) rc = xq_trainer_learn_apply(t, world);
    }
    const int rc_off = xq_dqn_set_fused_apply(t->dqn, fused_before);     // also after a failed iteration
    return rc != XQ_OK ? rc : rc_off;
}

int xq_trainer_counters(xq_trainer* t, uint64_t* env_steps, uint64_t* updates, uint64_t* episodes) {
    if (!t) return fail(XQ_ERR_INVALID_ARGUMENT, "null trainer");
    if (env_steps) *env_steps = t->env_steps;
    if (updates) *updates = t->updates;
    if (episodes) {
        unsigned long long head = 0;
        if (t->cstream) XQ_HIP(hipStreamSynchronize(t->cstream));
        XQ_HIP(hipStreamSynchronize(t->stream));
        XQ_HIP(hipMemcpy(&head, t->env->ep_head, sizeof head, hipMemcpyDeviceToHost));
        *episodes = head;
    }
    return XQ_OK;
}

}  // extern "C"
