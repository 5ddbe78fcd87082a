/* xq_capi.h — C ABI of libxqhip.so, the MI355X-native (gfx950) batched Xiangqi self-play + DQN hot path.
 *
 * This is the drop-in boundary for the training path of Qervas/cn_chess_ai (reference @ 2024-10-20).  The reference
 * has no FFI layer: its boundary is the C++ class surface ChessBoard / ChessAI / DQN / NeuralNetwork.  Every entry
 * point below names the reference interface it replaces (file:line into the reference tree); the C++ facade in
 * include/xq/ rebuilds those classes on top of this ABI, and INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *   - opaque handles, plain pointers and sizes, no C++ or torch types;
 *   - every function returns an xq_status (0 = ok) and never throws; xq_last_error() gives the message of the last
 *     failure on the calling thread;
 *   - pointers named *_host are caller-owned host memory, *_dev are device (HBM) pointers on the handle's device;
 *   - each handle runs on ONE hipStream_t (passed as void*; NULL = a stream the handle creates); calls are
 *     asynchronous on that stream unless they return data to the host, in which case they synchronise that stream;
 *   - handles that exchange DEVICE data are ordered by stream order when they were created on the same stream — what xq_trainer
 *     does, and the simplest way to use the ABI.  For handles on streams of their own see "Stream ordering" below: whatever is passed
 *     as a HANDLE the library orders itself, whatever is passed as a raw device pointer is the caller's to order;
 *   - handles are not thread-safe; one GPU per process (one rank per GPU under torch.distributed / RCCL).
 *
 * Stream ordering (no upstream analogue: the reference has one stream and a cudaDeviceSynchronize() after every launch).  Every pair of
 * entry points through which two handles hand each other device data, and what orders the consumer behind the producer when the two
 * handles run on different streams (same stream: stream order, nothing recorded).  "library" = the ring keeps, per resource, the
 * stream of the last write and of the reads since, and the consumer's stream waits on an event recorded on the producer's stream
 * (cn_chess_ai_amd/csrc/xq_internal.h, SharedResource); each class can be switched off with xq_debug_set_stream_ordering for the test
 * that shows it is needed (tests/test_stream_order_gpu.py: every row below has a sync-vs-nosync case that goes red without it).
 *
 *   producer -> consumer                                         device data                       ordered by
 *   xq_env_selfplay_step(replay) -> xq_dqn_td_grads_replay        ring slots (s, a, r, s', done)    library: XQ_ORDER_RING_CONTENTS
 *   xq_dqn_td_grads_replay -> xq_env_selfplay_step(replay)        the slots that step still reads   library: XQ_ORDER_RING_CONTENTS
 *   xq_env_selfplay_step(replay) -> xq_replay_get                 ring slots                        library: XQ_ORDER_RING_CONTENTS
 *   xq_env_selfplay_step(replay) -> xq_replay_per_rebuild         priorities of new transitions     library: XQ_ORDER_RING_PRIORITIES
 *   xq_dqn_td_grads_replay (prioritized) -> xq_replay_per_rebuild TD-error priorities               library: XQ_ORDER_RING_PRIORITIES
 *   xq_replay_per_rebuild -> xq_env_selfplay_step(replay)         maximum-priority snapshot         library: XQ_ORDER_RING_PRIORITIES
 *   xq_replay_per_rebuild -> xq_replay_sample_prioritized         sum tree                          one stream (the ring's): stream order
 *   xq_replay_sample* -> xq_dqn_td_grads_replay                   slot list, importance weights     library: XQ_ORDER_RING_DRAW
 *   xq_dqn_td_grads_replay -> next xq_replay_sample*              the list that step still reads    library: XQ_ORDER_RING_DRAW
 *   xq_dqn_apply_grads / set_params / load_model / update_target
 *     -> xq_dqn_forward* / select_q_dev / td_grads*               parameters                        one handle, one stream: stream order
 *     -> xq_trainer_collect (collect stream of overlap_collect)   parameters                        library: XQ_ORDER_TRAINER_PARAMS
 *   opponent net (xq_trainer_set_opponent) -> xq_trainer_collect  its Q rows of the trainer's boards   library: events (the forward on
 *                                                                 (and the boards it reads)           the net's stream waits for the env)
 *   xq_dqn_select_q_dev / forward_boards_dev -> xq_env_selfplay_step   q90_dev (raw pointer)        CALLER: xq_stream_wait_stream(env stream, Q-net stream)
 *   xq_env_*step* -> xq_dqn_select_q_dev / forward_boards_dev / td_grads(boards_dev)  boards (raw pointer)   CALLER: xq_stream_wait_stream(Q-net stream, env stream)
 *   xq_env_selfplay_step(results_dev) / legal_moves_dev -> anything    raw pointers                 CALLER
 *   xq_comm_allreduce(buf_dev, stream), xq_allreduce_grads        caller's buffer / gradient buffer on the stream given / the handle's: stream order
 *   host-buffer entry points (*_host, set_state, get_*, push_host, set_priorities, set_params, backpropagate)   synchronise before they return
 * A stream handed to a handle must outlive every handle that exchanged data with it (events are recorded on it lazily).
 *
 * Encodings
 *   - square  s = row*9 + col, rows 0..9 (Red home rows 0-4, Red moves +row: chessboard.cpp:12-28), cols 0..8;
 *   - piece code: 0 empty, 1..7 = Red General,Advisor,Elephant,Horse,Chariot,Cannon,Soldier, 8..14 = Black
 *     (PieceType/PieceColor, chessboard.h:8-14; code-1 is the one-hot plane of chessai.cpp:278-282);
 *   - a board given on the host (xq_env_set_state, xq_replay_push_host) holds codes 0..14 and AT MOST 16 PIECES OF ONE COLOUR, of any
 *     types on any squares; anything else is XQ_ERR_INVALID_ARGUMENT and nothing is written.  (The move generator ranks a side's
 *     pieces into a 16-entry table; play from the start position never has more.)  A move list holds XQ_MAX_MOVES = 128 entries: a
 *     side with more moves — only such arbitrary boards can have them — gets the first 128 in canonical order, count 128;
 *   - action code = from*90 + to  (Action{from,to}, action.h:4-11);
 *   - colours: 0 Red, 1 Black, 2 None (PieceColor, chessboard.h:12-14).
 */
#ifndef XQ_CAPI_H
#define XQ_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    XQ_OK = 0,
    XQ_ERR_INVALID_ARGUMENT = 1,  /* std::invalid_argument upstream (dqn.cu:17-19,200,324-329) */
    XQ_ERR_RUNTIME = 2,           /* std::runtime_error upstream: device error (dqn.h:16-24), empty action list (dqn.cpp:26-28) */
    XQ_ERR_NO_DEVICE = 3,         /* no gfx950 device / HIP runtime unusable: the product path has NO CPU fallback */
    XQ_ERR_IO = 4,                /* model file open/read/write failure or layer mismatch (dqn.cpp:80,115,147) */
    XQ_ERR_UNDEFINED_UPSTREAM = 5 /* bug-compatible backprop requested for a topology where the reference reads out of bounds */
} xq_status;

enum { XQ_MAX_MOVES = 128, XQ_BOARD_WORDS = 12, XQ_MAX_LAYERS = 8 };

const char* xq_last_error(void);
int xq_version(void);
/* Device plumbing (replaces the implicit cudaMalloc/cudaDeviceSynchronize device of dqn.cu). */
int xq_device_count(int* n);
int xq_set_device(int device);
int xq_stream_synchronize(void* hip_stream);
/* A HIP stream for callers that have no HIP headers of their own (the ctypes binding, the C++ facade): priority -1 urgent, 0 normal,
 * 1 background (streams of different priority never share a hardware queue; streams of one priority may, and then run in submission
 * order); nonblocking != 0: not ordered against the legacy null stream.  Destroy it after the handles that run on it. */
int xq_stream_create(int priority, int nonblocking, void** hip_stream);
int xq_stream_destroy(void* hip_stream);
/* Orders everything queued on waiting_stream from now on behind everything queued on producer_stream so far (one event record + one
 * wait; no host synchronisation) — for the device pointers the caller hands from one handle to another ("Stream ordering" above). */
int xq_stream_wait_stream(void* waiting_stream, void* producer_stream);
/* idle = 1 when everything queued on the stream so far has completed (hipStreamQuery), without blocking. */
int xq_stream_query(void* hip_stream, int* idle);
/* Diagnostics of the ordering tests — REFUSED (XQ_ERR_INVALID_ARGUMENT) unless the process runs with XQ_DEBUG_API=1 in its environment:
 * they stall streams and switch the library's synchronisation off.
 * xq_debug_stream_gate queues a one-wave kernel on hip_stream that waits until the HOST calls xq_debug_gate_release (or timeout_ms, 1..5000,
 * have passed: the kernel always ends): whatever is queued behind it is late by construction, not by a guess about durations.
 * xq_debug_gate_destroy after the stream has been synchronised.  xq_debug_stream_delay queues a kernel that spins for `microseconds`
 * (<= 200000).  xq_debug_set_stream_ordering: bit mask of the ordering classes the library provides (default XQ_ORDER_ALL);
 * process-wide; setting it back to XQ_ORDER_ALL is always allowed. */
enum { XQ_ORDER_RING_CONTENTS = 1, XQ_ORDER_RING_PRIORITIES = 2, XQ_ORDER_RING_DRAW = 4, XQ_ORDER_TRAINER_PARAMS = 8, XQ_ORDER_ALL = 15 };
int xq_debug_stream_gate(void* hip_stream, int timeout_ms, void** gate);
int xq_debug_gate_release(void* gate);
int xq_debug_gate_destroy(void* gate);
int xq_debug_stream_delay(void* hip_stream, int microseconds);
int xq_debug_set_stream_ordering(unsigned mask);
/* HIP-event timing on a given stream, for bench.py's roofline leg (ms between the two records). */
int xq_event_create(void** ev);
int xq_event_destroy(void* ev);
int xq_event_record(void* ev, void* hip_stream);
int xq_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);

/* ------------------------------------------------------------------------------------------------------------
 * xq_env — thousands of ChessBoard instances resident in HBM (chessboard.h:35-78), one wavefront per board.
 * HBM layout per game: board = 12 x u32 (90 squares x 4 bit), meta = 4 x u32
 *   {moveCount | player<<16, redScore | blackScore<<16, plies played by this slot (RNG counter), episodes finished}.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct xq_env xq_env;

/* ChessBoard::ChessBoard() x n_games (chessboard.cpp:4-6).  game ids are first_game_id .. +n_games-1 (RNG streams). */
int xq_env_create(int n_games, uint64_t seed, uint32_t first_game_id, void* hip_stream, xq_env** out);
int xq_env_destroy(xq_env* env);
int xq_env_num_games(const xq_env* env, int* n);
int xq_env_stream(const xq_env* env, void** hip_stream);      /* the stream the handle runs on (its own when it was created with NULL) */
/* ChessBoard::reset() on every game (chessboard.cpp:95-102); also zeroes the RNG counters and episode counts. */
int xq_env_reset(xq_env* env);
/* Test/interop access to the state (no upstream analogue: upstream board is private).  boards90: [n][90] piece codes;
 * meta4: [n][4] = moveCount, currentPlayer, redScore, blackScore (chessboard.h:62-77).  A board with a code above 14 or with more
 * than 16 pieces of one colour is rejected (XQ_ERR_INVALID_ARGUMENT, no game changed). */
int xq_env_set_state(xq_env* env, int first, int n, const uint8_t* boards90_host, const int32_t* meta4_host);
int xq_env_get_state(xq_env* env, int first, int n, uint8_t* boards90_host, int32_t* meta4_host);
/* ChessAI::getAllValidActions(player) for every game (chessai.cpp:347-368 over chessboard.cpp:112-283): canonical
 * order (from ascending, then generator order).  player: 0 Red, 1 Black, -1 = each game's side to move.
 * codes: [n_games][128] u16 action codes, counts: [n_games]. */
int xq_env_legal_moves(xq_env* env, int player, uint16_t* codes_host, int32_t* counts_host);
int xq_env_legal_moves_dev(xq_env* env, int player, uint16_t* codes_dev, int32_t* counts_dev);
/* Material search of every game for its side to move (build-defined, DESIGN.md §4 "Search player"): a full-width negamax of
 * depth 1, 2 or 3 plies over the xq_env_legal_moves list, int32 values in material points, XQ_SEARCH_MATE - k for a general
 * captured k plies from the root.  values: [n_games][128] root value of each move in list order (INT32_MIN past the count),
 * counts: [n_games] move counts, best: [n_games] index of the first best move (-1 without a move).  Any other depth:
 * INVALID_ARGUMENT.  The _dev form writes device buffers on the env's stream and does not synchronise. */
enum { XQ_SEARCH_MATE = 1000000 };
int xq_env_search(xq_env* env, int depth, int32_t* values_host, int32_t* counts_host, int32_t* best_host);
int xq_env_search_dev(xq_env* env, int depth, int32_t* values_dev, int32_t* counts_dev, int32_t* best_dev);
/* ChessBoard::getWinner() (chessboard.cpp:312-320) for games first..first+n-1: colour of the first general in index order
 * (so Red while both are alive), 2 if none. */
int xq_env_get_winner(xq_env* env, int first, int n, uint8_t* winners_host);
/* ChessBoard::isValidMove for all 90x90 (from,to) pairs of game g (chessboard.cpp:66-93,328-440): valid8100[f*90+t]. */
int xq_env_valid_matrix(xq_env* env, int game, uint8_t* valid8100_host);

/* The seven public per-piece validators isValid{General,Advisor,Elephant,Horse,Chariot,Cannon,Soldier}Move
 * (chessboard.h:50-56, chessboard.cpp:328-440) of game g, evaluated on device as upstream writes them (geometry + occupancy
 * only; the piece on `from` is not consulted except for the soldier's colour): rules[(type-1)*8100 + f*90 + t] for all in-board
 * (from, to) pairs, type = PieceType 1..7.  xq_env_rule_query answers one call with arbitrary coordinates (upstream reads
 * squares outside the board as Empty); from == to on a chariot/cannon overflows a loop upstream => XQ_ERR_UNDEFINED_UPSTREAM. */
int xq_env_rule_matrix(xq_env* env, int game, uint8_t* rules7x8100_host);
int xq_env_rule_query(xq_env* env, int game, int piece_type, int from_row, int from_col, int to_row, int to_col, int* ok);

/* Per-game result of one ply.  Mirrors what chessai.cpp:113-119,146-162 derives after movePiece(). */
typedef struct {
    int32_t action;      /* action code played, -1 if the side to move had no action (chessai.cpp:100-103) */
    int32_t n_moves;     /* size of the legal list the action was chosen from (0 for xq_env_step) */
    int32_t reward;      /* evaluateBoard(mover, post-move count), chessai.cpp:311-345; where no move was made (action -1, or a
                          * rejected move of xq_env_step) it is evaluateBoard(side to move, the unchanged count) of the untouched board.
                          * Always evaluateBoard, part of the ABI: xq_env_set_reward changes what a replay ring gets, never this field */
    uint8_t captured;    /* piece code movePiece() returned (chessboard.cpp:38-64); 0 = none or invalid move */
    uint8_t valid;       /* 0: movePiece() rejected the move — no state change */
    uint8_t done;        /* checkGameOver() || moveCount+1 >= 200 (chessai.cpp:119) */
    uint8_t terminated;  /* episode ended: checkGameOver() (chessboard.cpp:286-309) or no action; board was auto-reset */
    uint8_t winner;      /* getWinner() (chessboard.cpp:312-320) when terminated, else 2 */
    uint8_t explored;    /* 1: epsilon branch taken (dqn.cpp:31-34); 2: a Boltzmann draw (xq_env_set_policy) played another move than
                          * the first maximum; else 0 */
    uint16_t move_count; /* getMoveCount() after the move (before auto-reset) */
    int16_t red_score, black_score; /* getRedScore()/getBlackScore() after the move (before auto-reset) */
} xq_step_result;

/* ChessBoard::movePiece with caller-chosen actions (chessboard.cpp:38-64) + evaluateBoard + checkGameOver, per game.
 * actions: [n_games] action codes (any int; out-of-board / invalid => rejected, no state change).
 * auto_reset != 0: a game whose checkGameOver() became true BY THIS MOVE is reset (the `for episode` loop of chessai.cpp:89-90).
 * A rejected move changes nothing — no counters, no episode record, no reset — also on an already finished board
 * (its result still reports terminated/winner: that is how the facade's checkGameOver() probes). */
int xq_env_step(xq_env* env, const int32_t* actions_host, int auto_reset, xq_step_result* results_host);

/* One self-play ply for every game, fully on device: legal moves (LDS) -> epsilon-greedy DQN::selectAction
 * (dqn.cpp:24-56; q90_dev = tanh Q-values of outputs 0..89 per game, row stride q_stride floats; NULL = uniform random
 * policy) -> movePiece -> evaluateBoard -> done -> auto-reset.  rand() is replaced by Philox4x32-10
 * (ctr = {ply counter of the slot, 0, game id, 0}, key = seed): explore iff r0 < eps_u32, index = r1 % n.
 * results_dev: optional [n_games] xq_step_result in HBM; replay: optional ring that receives the transition. */
typedef struct xq_replay xq_replay;
int xq_env_selfplay_step(xq_env* env, const float* q90_dev, int q_stride, uint32_t eps_u32,
                         xq_step_result* results_dev, xq_replay* replay);
/* Convenience for tests: same, copying results to the host. */
int xq_env_selfplay_step_host(xq_env* env, const float* q90_host, uint32_t eps_u32, xq_step_result* results_host);

/* The reward the env kernel writes into a replay ring (DESIGN.md §4 "Reward rule") — build-defined; the default is the reference's.
 *   XQ_REWARD_EVALUATE : evaluateBoard(mover, moveCount) (chessai.cpp:115, :311-345; versus training: from the learner's side): the
 *                        absolute material balance, up to +-1480, minus a truncated 0.1 moveCount.  Same launches and bits as an env that
 *                        was never asked; scale, ply_cost and bound are checked, kept and not used.
 *   XQ_REWARD_DELTA    : the change of material balance over the transition, scaled, less a cost per ply, clamped.  With B(board, side) =
 *                        the PieceScore sum of side's pieces minus the other side's (general 1000; evaluateBoard's material sum):
 *                          self-play: delta = B(s', mover) - B(s, mover)      = the value of the piece this ply took (>= 0)
 *                          versus   : delta = B(s', learner) - B(s, learner)  = what the learner took minus what the reply took, over the
 *                                     whole learner transition; the game ended by the learner's move: its part only; the empty slot of
 *                                     an opponent's pre-move that ended the game keeps reward 0
 *                          r = min(max(fl32(fl32((float)delta * (float)scale) - (float)ply_cost), -(float)bound), (float)bound)
 *                        in fp32, one rounding per operation.  A row without an action (action_to -1) stays an empty row: delta = 0 there.
 *                        The gain is the captured piece's value, not a difference of tracked scores, so boards from xq_env_set_state
 *                        follow the same rule.
 * As fp32 values: scale finite and > 0, ply_cost finite and >= 0, bound > 0 (+inf: no clamp); anything else, NaN included, or an unknown
 * kind: XQ_ERR_INVALID_ARGUMENT and nothing changes.  Takes effect at the next launch that writes a ring (xq_env_selfplay_step with a
 * replay, a trainer's collect); slots already written keep their values.  xq_step_result.reward, host pushes and the arena are untouched.
 * xq_env_get_reward: the values as last given — on an env that was never asked XQ_REWARD_EVALUATE, 1e-3, 0, 1.  Outputs may be NULL. */
enum { XQ_REWARD_EVALUATE = 0, XQ_REWARD_DELTA = 1 };
int xq_env_set_reward(xq_env* env, int kind, double scale, double ply_cost, double bound);
int xq_env_get_reward(const xq_env* env, int* kind, double* scale, double* ply_cost, double* bound);

/* How a ply that reads Q rows and did NOT take the epsilon branch picks its move (DESIGN.md §4 "Exploration policy") — build-defined; the
 * default is the reference's.
 *   XQ_POLICY_GREEDY    : the first maximum of q[action.to] over the legal list (dqn.cpp:39-51).  Same launches and bits as an env that
 *                         was never asked; the temperature is checked, kept and not used.
 *   XQ_POLICY_BOLTZMANN : a softmax draw over the values v_i the greedy pick compares (q[to_i]; q[swap(to_i)] for Black under
 *                         xq_env_set_q_view; NaN counts as -inf), list order i = 0..n-1.  m = max v_i; if m is not finite (every
 *                         candidate -inf or NaN, or a +inf present) the pick is the first maximum.  Otherwise, in fp32 with one rounding
 *                         per operation, x_i = fl(fl(v_i - m) * it), it = (float)(1.0 / temperature), w_i = expf(x_i) (0 where v_i =
 *                         -inf), u = (r2 >> 8) * 2^-24 on word 2 of the ply's Philox block (r0: epsilon, r1: the uniform index),
 *                         t = u * sum w: the first i whose inclusive running sum exceeds t, or the last i with w_i > 0 if rounding
 *                         leaves none.  tests/boltzmann_ref.py is the definition, with the band inside which the device's expf and
 *                         summation order may resolve a draw either way.
 * The epsilon branch (r0 < eps_u32: move r1 % n), a ply without Q rows, the search players' picks and the arena's opening are untouched.
 * xq_step_result.explored is 2 where the draw played another move than the first maximum; xq_env_counters[5] counts epsilon plies only.
 * temperature as fp32 must be finite and in [1e-3, 1e3]; anything else, NaN included, or an unknown kind: XQ_ERR_INVALID_ARGUMENT and
 * nothing changes.  Takes effect at the next xq_env_selfplay_step* or trainer collect on the env; versus training: the learner's
 * half-ply only, the opponent stays epsilon-greedy.  xq_env_get_policy: the values as last given — on an env that was never asked
 * XQ_POLICY_GREEDY, 1.  Outputs may be NULL. */
enum { XQ_POLICY_GREEDY = 0, XQ_POLICY_BOLTZMANN = 1 };
int xq_env_set_policy(xq_env* env, int kind, double temperature);
int xq_env_get_policy(const xq_env* env, int* kind, double* temperature);

/* Episode reporting — the gameCompleted(game, redScore, blackScore) signal (chessai.h:35, chessai.cpp:162). */
typedef struct {
    uint32_t game_id, episode;   /* episode = 1-based count for that game slot (signal's `gameNumber`) */
    int16_t red_score, black_score;
    uint16_t move_count;
    uint8_t winner, reserved;
} xq_episode_record;
/* Drains up to max_records finished-episode records (oldest first); *n_out = number written, *total = episodes so far.
 * The env keeps the newest max(4096, 4 * n_games) records that have not been drained: when more than that finish between two
 * drains the oldest are dropped (the next drain starts at the oldest record still there) and *total still counts them.  A record is
 * written at most once: what one call leaves (max_records reached) the next returns.  max_records <= 0 or records_host == NULL: *n_out =
 * 0 and *total only, and nothing is lost that the ring still holds.  xq_env_reset empties the ring: *total and the episode numbers of
 * every game slot start again. */
int xq_env_drain_episodes(xq_env* env, xq_episode_record* records_host, int max_records, int* n_out, uint64_t* total);
/* totals since create/reset: [0] plies, [1] episodes, [2] red wins, [3] black wins, [4] captures, [5] explored plies */
int xq_env_counters(xq_env* env, uint64_t counters6_host[6]);
const uint32_t* xq_env_boards_dev(const xq_env* env);   /* [n_games][12] packed boards in HBM */
const uint32_t* xq_env_meta_dev(const xq_env* env);     /* [n_games][4] */

/* ------------------------------------------------------------------------------------------------------------
 * xq_replay — ReplayBuffer of N7's 5-tuple (state, action.to, reward, nextState, done), dqn.cpp:157-172.
 * Not in the reference (SURVEY §8b "New"): ring in HBM, states stored as packed boards (48 B), never as 1260 floats.
 * ---------------------------------------------------------------------------------------------------------- */
int xq_replay_create(int capacity, uint64_t seed, void* hip_stream, xq_replay** out);
int xq_replay_destroy(xq_replay* r);
int xq_replay_size(xq_replay* r, int* size, int* capacity, uint64_t* total_pushed);
int xq_replay_stream(const xq_replay* r, void** hip_stream);
/* push(s, a, r, s', done) for n transitions given as 90-byte boards on the host (tests / interop).  Boards as xq_env_set_state:
 * a code above 14 or more than 16 pieces of one colour in s or s' is XQ_ERR_INVALID_ARGUMENT and nothing is pushed. */
int xq_replay_push_host(xq_replay* r, int n, const uint8_t* boards90, const int32_t* action_to, const float* reward,
                        const uint8_t* done, const uint8_t* next_boards90);
/* sample(B): uniform with replacement, Philox(ctr = {draw, 0, sample call #, 1}, key = seed) % size.
 * Returns the chosen slots; xq_dqn_td_grads_replay consumes them on device.  Streams: the draw runs on the ring's stream, the
 * consumer on the Q-net's, env steps that fill the ring on the env's.  When those differ the library orders them itself ("Stream
 * ordering" at the top) — the TD step waits for the draw and for the env steps that wrote the ring, the next draw (it overwrites the
 * slot list) and the next env step (it overwrites slots) wait for the TD step that still reads them — so a caller may draw, queue the
 * step, play and draw again without synchronising.  (xq_trainer orders its own ring by hand: its collects write slots that the TD
 * step running beside them never samples, xq_replay_sample_window.) */
int xq_replay_sample(xq_replay* r, int batch, int32_t* slots_host /* optional */);
/* sample(B) restricted to the `count` ring slots that start at `start` (wrapping): slot = (start + Philox % count) % capacity.
 * The overlapped trainer uses it to leave out the slots a concurrent collect is writing; (0, size) == xq_replay_sample. */
int xq_replay_sample_window(xq_replay* r, int batch, int start, int count, int32_t* slots_host /* optional */);
int xq_replay_get(xq_replay* r, int slot, uint8_t* board90, int32_t* action_to, float* reward, uint8_t* done,
                  uint8_t* next_board90);
/* Prioritized replay, proportional variant (Schaul et al., ICLR 2016) — build-defined (BASELINE configs[4]), defined by
 * DESIGN.md §4:  p_i = (|TD error_i| + eps)^alpha, P(i) = p_i / sum p, stratified draw of one sample per segment of
 * the total mass (Philox ctr = {k, 0, sample call #, 2}), importance weight w_i = (N * P(i))^-beta / max_batch w applied to the
 * sample's gradient, new transitions enter with the largest priority assigned so far.  The masses live in a radix-32 sum tree in
 * HBM whose nodes are sequential fp32 sums (fixed association: sampled slots are reproducible bit for bit).
 *   xq_replay_enable_per      : once, before use (allocates the priority table and the tree)
 *   xq_replay_per_rebuild     : zeroes the priorities of `retire_count` slots from `retire_start` (wrapping; slots about to be
 *                               overwritten), rebuilds the tree from the priority table and snapshots the running maximum
 *   xq_replay_sample_prioritized: draws `batch` slots from the tree as of the last rebuild; xq_dqn_td_grads_replay then applies the
 *                               importance weights and writes the new priorities of the sampled slots back
 *   set/get_priorities, per_stats: tests / interop
 * Call order: rebuild -> sample_prioritized -> td_grads_replay.  A rebuild between a draw and its TD step is allowed (the batch maximum
 * of the draw's importance weights is left alone until the step has been queued). */
int xq_replay_enable_per(xq_replay* r, double alpha, double beta, double eps);
int xq_replay_per_rebuild(xq_replay* r, int retire_start, int retire_count);
int xq_replay_sample_prioritized(xq_replay* r, int batch, int32_t* slots_host /* optional */, float* weights_host /* optional, normalised */);
int xq_replay_set_priorities(xq_replay* r, int first, int n, const float* prio_host);
int xq_replay_get_priorities(xq_replay* r, int first, int n, float* prio_host);
int xq_replay_per_stats(xq_replay* r, float* total, float* max_priority, int* n_eligible);
/* xq_replay_per_rebuild with a hold window: the `hold_count` slots from `hold_start` (wrapping) count as priority 0 in the snapshot the
 * sampler reads and in the sums of the tree ONLY — they are never drawn and are not among n_eligible, while the live priority table
 * keeps their values, so a later rebuild without them in its hold makes them eligible with the priority they had.  n-step returns hold
 * the newest (n_step - 1) * stride slots, whose chains are not complete yet.  xq_replay_per_rebuild is this call with a hold of 0:
 * the same launches, the same bits.  A window outside the ring is XQ_ERR_INVALID_ARGUMENT. */
int xq_replay_per_rebuild_hold(xq_replay* r, int retire_start, int retire_count, int hold_start, int hold_count);
/* n-step TD returns (DESIGN.md §4 "n-step returns") — build-defined, off by default.  With n_step > 1 every xq_dqn_td_grads_replay from
 * this ring first assembles, per minibatch row, the n-step transition that starts at the sampled slot, and then runs the TD step it always
 * ran on that batch, with the discount gamma^n.
 *   The ring has capacity `cap`; successive transitions of one trajectory lie `stride` slots apart in age order (xq_env_selfplay_step
 *   writes game g of a collect to slot write_pos + g: stride = the number of games).  The readable range is `count` slots in age order
 *   from slot `first`: first = 0 while the ring is not full and the write position once it is, count = the filled size (xq_trainer narrows
 *   it, see xq_trainer_set_n_step).  For row b with sampled slot s: off0 = (s - first) mod cap; chain element k (0 <= k < n) lives at
 *   off_k = off0 + k * stride, slot (first + off_k) mod cap, and exists iff off_k < count.
 *   Arithmetic is fp32, one rounding per operation, no fma: gf = (float)gamma, disc_0 = 1, disc_k = fl32(disc_{k-1} * gf) (host).
 *   R = r_0, D = done_0, m = 1; for k = 1 .. n-1 while !D: if element k does not exist or its action_to < 0 the row is DEAD and the scan
 *   stops; otherwise R = fl32(R + fl32(disc_k * r_k)), D = done_k, m = k + 1.  A row whose own action_to < 0 is dead as it is today (no
 *   scan: m = 1).  A chain that reaches `done` before it would leave the readable range is live.
 *   Staged transition: board = boards[s], next_board = next_boards[slot_{m-1}], action = dead ? -1 : a_0, reward = R, done = D.  A dead
 *   row stages s's own two boards; it contributes no gradient and loss 0 and keeps its priority (the rule of an empty slot).
 *   TD step on the staged batch: y = D ? R : R + disc_n * tanh(max) — !D implies m == n, so this is the n-step target.  A prioritized
 *   draw gets its importance weights as always; the TD-error priorities go back to the sampled slots behind the step.
 * n_step == 1 is off: the kernels, launches and bits of a ring that was never asked.  XQ_ERR_INVALID_ARGUMENT for n_step outside
 * 1..XQ_MAX_N_STEP, stride outside 1..capacity, or (n_step - 1) * stride >= capacity.  Takes effect at the next xq_dqn_td_grads_replay;
 * xq_dqn_td_grads with raw pointers is never affected.  In self-play the chain follows consecutive plies of one game — both sides'
 * moves, the one-trajectory view ChessAI::train takes of them (chessai.cpp:121-133); in versus training it is the learner's own
 * trajectory. */
enum { XQ_MAX_N_STEP = 8 };
int xq_replay_set_n_step(xq_replay* r, int n_step, int stride);
int xq_replay_get_n_step(const xq_replay* r, int* n_step /* optional */, int* stride /* optional */);
/* Mirror augmentation (DESIGN.md §4 "Mirror augmentation") — build-defined, off by default.  Xiangqi is symmetric under the left-right
 * reflection col -> 8 - col, so the reflection of a played transition is as true as the transition.  While prob > 0 every
 * xq_dqn_td_grads_replay from this ring stages its minibatch in the handle's staging buffers (the n-step ones) and reflects the rows
 * whose flag is set; the TD step it always ran then runs on the staged batch.  The ring is never written.
 *   flag_b = (prob == 1) || philox4x32_10(ctr = {b, 0, call, 3}, key = ring seed).v[0] < floor(prob * 2^32), saturated (the threshold
 *   rule of the env's epsilon).  Counter word 3 keeps the stream apart from the draw (1) and the stratified draw (2).  `call` counts the
 *   mirror-mode TD steps queued from this ring since it was created (the first is 0; steps taken while prob == 0 do not count).  The
 *   flag depends on the row alone: not on the slot, on whether the row is live, or on how the batch was drawn (explicit slots, the
 *   trainer's implicit draw, the identity of batch = 0, a prioritized draw).
 *   A flagged row: board'[r * 9 + c] = board[r * 9 + (8 - c)] for s and s' (nibbles 90..95 stay 0); action a' = a - 2 (a mod 9) + 8
 *   when 0 <= a < 90, any other value (-1: dead or empty, 90..95) as it is; reward and done unchanged.  Dead and empty rows follow the
 *   same flag rule and still contribute nothing.  An unflagged row is the sampled transition bit for bit.
 *   The step: identity slot source on the staged batch; with n_step == 1 the discount is (float)gamma as always; a prioritized draw
 *   gets its importance weights as always and the priorities of its live rows go back to the SAMPLED slots behind the step.  With
 *   n_step > 1 the n-step batch is assembled first and the flag applies to the assembled transition: s, the staged s' and a_0.
 * prob == 0 is off: the kernels, launches and bits of a ring that was never asked.  NaN or a value outside [0, 1] is
 * XQ_ERR_INVALID_ARGUMENT.  Takes effect at the next xq_dqn_td_grads_replay; xq_dqn_td_grads with raw pointers, xq_dqn_td_update_host
 * and xq_dqn_backpropagate are never affected.  The setting lives on the ring: it survives xq_dqn_set_optimizer, set_params, a model
 * load, a target update and xq_replay_set_n_step. */
int xq_replay_set_mirror(xq_replay* r, double prob);
int xq_replay_get_mirror(const xq_replay* r, double* prob /* optional */, uint64_t* calls /* optional: the `call` the next mirror-mode step will use */);
/* Colour-swap augmentation (DESIGN.md §4 "Colour-swap augmentation") — build-defined, off by default; the mirror's sibling.  Xiangqi is
 * also symmetric under exchanging the colours while turning the board top to bottom (row -> 9 - row): the same position with Red and
 * Black exchanged is the same game for the other side, so (swap(s), swap(a), r, swap(s'), done, 1 - side) is as true as the transition
 * that was played.  While prob > 0 every xq_dqn_td_grads_replay from this ring stages its minibatch in the handle's staging buffers and
 * transforms the rows whose flag is set; the TD step it always ran then runs on the staged batch.  The ring is never written.
 *   flag_b = (prob == 1) || philox4x32_10(ctr = {b, 0, call, 4}, key = ring seed).v[0] < floor(prob * 2^32), saturated (the threshold
 *   rule of the env's epsilon).  Counter word 4 keeps the stream apart from the draw (1), the stratified draw (2) and the mirror (3).
 *   `call` is a counter of its own: the colour-swap-mode TD steps queued from this ring since it was created (the first is 0; steps
 *   taken while prob == 0 do not count; the mirror's counter is untouched).  The flag depends on the row index alone.
 *   A flagged row: board'[(9 - r) * 9 + c] = sigma(board[r * 9 + c]) for s and s', with sigma(0) = 0, sigma(x) = x + 7 for 1..7 and
 *   sigma(x) = x - 7 for 8..14 (nibbles 90..95 stay 0); action a' = a + 81 - 18 (a div 9) when 0 <= a < 90, any other value (-1: dead or
 *   empty, 90..95) as it is; reward and done unchanged; under the legal-move bootstrap (xq_dqn_set_td_bootstrap) the staged side byte
 *   becomes 1 - side, taken after the n-step and mirror rules have chosen which slot's byte it is.  Dead and empty rows follow the same
 *   flag rule and still contribute nothing.  An unflagged row is the sampled transition bit for bit.
 *   The step: identity slot source on the staged batch, the discount rules of the mirror and the n-step returns; a prioritized draw gets
 *   its importance weights as always and the priorities of its live rows go back to the SAMPLED slots behind the step.  With n_step > 1
 *   the n-step batch is assembled first and the flag applies to the assembled transition.  With the mirror on as well both apply, each by
 *   its own flags; they commute (the mirror acts on columns, this on rows and codes), so the staged batch is defined without an order.
 * prob == 0 is off: the kernels, launches and bits of a ring that was never asked (a ring with the mirror on keeps exactly the mirror's).
 * NaN or a value outside [0, 1] is XQ_ERR_INVALID_ARGUMENT.  Takes effect at the next xq_dqn_td_grads_replay; xq_dqn_td_grads with raw
 * pointers, the host entry points, xq_dqn_backpropagate, the arena and the single-board loops are never affected.  The setting lives on
 * the ring: it survives xq_dqn_set_optimizer, set_params, a model load, a target update, xq_replay_set_n_step and xq_replay_set_mirror. */
int xq_replay_set_colour_swap(xq_replay* r, double prob);
int xq_replay_get_colour_swap(const xq_replay* r, double* prob /* optional */, uint64_t* calls /* optional: the `call` the next colour-swap-mode step will use */);

/* ------------------------------------------------------------------------------------------------------------
 * xq_dqn — DQN (dqn.h:97-116) = qNetwork + targetNetwork (NeuralNetwork, dqn.h:42-95, dqn.cu), fp32 on MFMA.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct xq_dqn xq_dqn;

enum { XQ_NET_ONLINE = 0, XQ_NET_TARGET = 1 };
enum { XQ_BACKPROP_REFERENCE = 0,  /* bug-compatible hidden delta, dqn.cu:406-423 as written */
       XQ_BACKPROP_TEXTBOOK = 1 };
enum { XQ_TD_ONLINE_NET = 0,       /* max Q(s') from the ONLINE net — what ChessAI::train does (chessai.cpp:126-127) */
       XQ_TD_TARGET_NET = 1,       /* max Q(s') from the target net — DQN::train (dqn.cpp:166-167) */
       XQ_TD_DOUBLE = 2 };         /* Double DQN (build-defined, BASELINE configs[4]): a* = argmax_k Q_online(s')[k] over all outputs
                                    * (first maximum: from -inf at output 0 with a strict >, so of several equal maxima the lowest
                                    * output wins, +0 and -0 are equal, +inf wins like any value, a NaN never wins — output 0
                                    * included — and when nothing wins, all outputs NaN or -inf, a* = 0),
                                    * y = r + gamma * Q_target(s')[a*] */
enum { XQ_PRECISION_F32 = 0,       /* fp32 MFMA everywhere (the reference computes in fp64; north_star: fp32, Q within 1e-4) */
       XQ_PRECISION_BF16 = 1,      /* bf16 Q-net (build-defined, BASELINE configs[4]): forward passes on bf16 MFMA — weights and hidden
                                    * activations rounded to bf16 (RNE), fp32 accumulation, biases and outputs fp32; backward and SGD
                                    * in fp32 on the master weights */
       XQ_PRECISION_BF16_FULL = 2 };/* the same forward, and the dense products of the backward pass on bf16 MFMA too: the lower hidden deltas
                                    * take the bf16 weights and the upstream delta rounded to bf16, the hidden weight gradients the delta
                                    * rounded to bf16 and the (already bf16) activations; fp32 accumulation, fp32 deltas for the bias /
                                    * layer-0 / output-layer gradients, fp32 master weights and SGD (defined in DESIGN.md section 4) */

enum { XQ_QMAX_FULL = 0,           /* max_a' Q(s',a') of the TD target (chessai.cpp:126-127, dqn.cpp:166-167): every output in fp32 */
       XQ_QMAX_SCREENED = 1 };     /* the same fp32 maximum, found by exact screening: all outputs once on the bf16 matrix pipe with a
                                    * rigorous error bound, then only the outputs within the bound of the screened maximum again in
                                    * fp32.  The value returned is the maximum of fp32-evaluated outputs. */

/* DQN::DQN(layerSizes, lr, gamma) (dqn.cpp:12-20) -> NeuralNetwork ctor (dqn.cu:14-57): W ~ U(-0.05,0.05) from a
 * seeded generator, biases 0; target = copy of online.  layer_sizes[0] must be 1260 for the board-input fast path;
 * any sizes work through the dense-state entry points. */
int xq_dqn_create(const int* layer_sizes, int n_sizes, double learning_rate, double gamma, uint64_t seed,
                  void* hip_stream, xq_dqn** out);
int xq_dqn_destroy(xq_dqn* d);
int xq_dqn_stream(const xq_dqn* d, void** hip_stream);
/* XQ_PRECISION_*: arithmetic of the forward passes on packed boards (action select, TD targets, Q(s,a)).  The dense-state entry
 * points (xq_dqn_forward / xq_dqn_backpropagate: the reference's std::vector<double> API) always compute in fp32. */
int xq_dqn_set_precision(xq_dqn* d, int precision);
/* Layer 0 of the s' chain of a TD step (online TD rule, fp32 net; no upstream analogue — the reference evaluates every state from
 * scratch, dqn.cu:199-260).  0 (default): the sum over the occupied squares of s' in ascending square order, the reference's
 * i-ascending accumulation with the zeros skipped.  1: z1(s') = z1(s) - rows of the squares that changed + rows of what stands there
 * now (two squares for a move; boards more than 8 squares apart are gathered in full): one gather instead of two, a DIFFERENT
 * summation order (differences ~1e-7 on the activations, far inside the 1e-4 budget on Q).  bench.py switches it on.
 * The same switch covers the select chain of the self-play loop (xq_dqn_select_q_dev / xq_trainer_collect, fp32 net): its layer-0
 * sums are kept per game, and while the online parameters do not change — the plies of one update — the next ply's sums are
 * derived from the kept ones the same way (used when an update period has several plies; a game that ended is summed in full). */
int xq_dqn_set_l0_derive(xq_dqn* d, int on);
/* How the gradient half of xq_dqn_td_grads is queued (no upstream analogue: dqn.cu:323-467 launches one kernel per layer and waits
 * for each).  1 (default): as fused launches on the handle's stream — per hidden layer below the top one ONE grid that holds the blocks
 * of the delta product, of the weight-gradient product above it and (first time) of the output-layer sums, then ONE grid with the
 * layer-0 sums and the bias column sums.  Taken for every fp32 net whose backward products fit 64 x 64 tiles (all BASELINE nets at
 * 8192-16384 samples); bf16 nets and larger products run the same kernels one by one on two streams (critical chain + side stream,
 * three event records and a join), as does 0.  What happens to the partial sums the fused launches leave: with
 * xq_dqn_set_fused_apply on and no communicator they stay pending and xq_dqn_apply_grads adds them; otherwise ONE launch reduces them
 * into the gradient buffer on the handle's stream, and an attached communicator all-reduces that buffer in ONE collective behind it
 * (xq_dqn_set_comm).  The same switch covers the other fusion of the step's second half: with exact screening on a net whose last
 * hidden layer is 256 wide (uniform replay), the TD target / output delta / top hidden delta are computed inside the blocks of the
 * kernel that re-evaluates the screened maxima instead of by a launch of their own.  Results are bitwise identical either way. */
int xq_dqn_set_td_tail(xq_dqn* d, int on);
/* How the layer-0 weight gradient of a TD step (updateWeightsBiasesKernel on layer 0, dqn.cu:310-319, fed by the one-hot of
 * chessai.cpp:268-289) is computed.  1 (default; first hidden width a multiple of 64 and >= 256 samples, other shapes take 0): the dense
 * product one-hot^T x delta_0 on the bf16 matrix pipe, exact — the one-hot operand is 0 / 1 and delta_0 is split into three bf16 values per
 * fp32 (hi + mid + lo, every residual exact), products exact, fp32 accumulation.  0: per-(square, piece) segmented sums of delta rows on
 * the vector ALU.  Same value up to the summation order (both within a few fp32 ulp of an fp64 evaluation).  Measured at 8192 x 256
 * (round 5): 17 against 37 us alone, the headline step 0.1755 against 0.1833 ms. */
int xq_dqn_set_l0_grad_mode(xq_dqn* d, int mode);
/* Exact screening, second pass: groups whose two largest screened values both reach the threshold are re-evaluated WHOLE (32 rows).  Nets whose
 * trained rows dominate can ask for one such group for nearly every sample; the refine kernel then serves the groups that many samples of a block
 * share from LDS (activation rows of the block + the rows of up to three groups staged in one sweep; 145 KB of LDS, so only for launches of at most
 * one block per CU and a 256-wide last hidden layer).  mode -1 (default): on while the screen's own counters — read back every 32 screened steps —
 * show more than 0.25 whole groups per sample, off below 0.10; 0: never; 1: whenever the launch has room.  A speed switch: same bits either way. */
int xq_dqn_set_refine_stage(xq_dqn* d, int mode);
/* XQ_QMAX_*: how the TD step finds max_a' Q(s',a').  XQ_QMAX_SCREENED applies to fp32 nets with XQ_TD_ONLINE_NET / XQ_TD_TARGET_NET
 * whose last hidden width is a multiple of 64 and whose product is large enough for the persistent GEMM (>= 512 tiles of 128 x 128);
 * every other case silently keeps the full fp32 product.  Guard: every 32 screened steps the candidate counters are read back
 * asynchronously; when the screen leaves more than 24 candidate groups (or 1 whole group) per sample — a net whose outputs all lie
 * within the bf16 bound of each other — the next 512 TD steps run the full product, then the screen is tried again.
 * The guard in step numbers (S counts screened steps; a step that runs the full product does not count; tests/guard_model.py is this
 * rule as a program):
 *   - behind every screened step with S % 32 == 0 the counters are copied back, unless a copy is still pending;
 *   - a pending copy is evaluated at the top of the first TD step at which S % 32 == 0 again and S is not the S it was queued at, on
 *     everything counted between the previous evaluation and the copy: the copy of S = 32 at the top of the step behind S = 64 (window
 *     S = 1..32), that of S = 96 behind S = 128 (window S = 33..96), and so on — one decision per 64 screened steps;
 *   - over the limit, that TD step and the 511 behind it run the full product;
 *   - a decision never counts a step that ran before the end of the last hold.  The first screened step behind a hold — whether the
 *     hold ran out or xq_dqn_set_qmax_mode(XQ_QMAX_SCREENED) ended it, which switches the screen on at once — queues a copy
 *     whatever S is; that copy decides nothing: at the next S % 32 == 0 it becomes the start of the next window, and that boundary's own
 *     copy is queued behind it;
 *   - a larger batch that needs a larger counter array drops the pending copy (the totals are kept); a dropped copy of the kind above is
 *     queued again behind the next screened step.
 * So a net the screen cannot handle, asked to screen every step: TD steps 1..64 screen, 65..576 run the full product, 577..640 screen
 * (S = 65..128: the copy of S = 65 starts the window at S = 96, the copy of S = 96 — window S = 66..96 — is evaluated behind S = 128),
 * 641..1152 run the full product: 64 screened and 512 full steps per cycle.  A net made harmless during a hold is not held again.
 * stats[4] (xq_dqn_qmax_stats, synchronises): TD steps screened, samples, candidate (sample, 32-output group) pairs re-evaluated in fp32,
 * pairs whose whole group was re-evaluated. */
int xq_dqn_set_qmax_mode(xq_dqn* d, int mode);
int xq_dqn_qmax_stats(xq_dqn* d, uint64_t stats[4]);
/* The guard's own counters: how often it has switched a run of TD steps to the full product so far, and how many steps of the current
 * run are left (0 = the screen is on).  No synchronisation. */
int xq_dqn_qmax_guard(xq_dqn* d, uint64_t* fallbacks, int* hold_steps_left);
int xq_dqn_num_params(const xq_dqn* d, size_t* n_weights, size_t* n_biases);
/* host_weights / host_biases in the REFERENCE flat layout (row-major [out][in] per layer, layers concatenated,
 * dqn.cu:112-140), fp64 like upstream.  set = copyToDevice() (dqn.cu:480-485), get = copyFromDevice() (:487-492).  The optimizer
 * state (xq_dqn_set_optimizer) is not touched: a caller that replaces the parameters of a run decides about xq_dqn_reset_optimizer. */
int xq_dqn_set_params(xq_dqn* d, int which_net, const double* weights_host, const double* biases_host);
int xq_dqn_get_params(xq_dqn* d, int which_net, double* weights_host, double* biases_host);
/* DQN::getQValues / NeuralNetwork::forward (dqn.cpp:65-68, dqn.cu:199-260) for n dense states [n][layer_sizes[0]]
 * -> q [n][layer_sizes[last]], fp64 at the boundary like upstream (computed in fp32). */
int xq_dqn_forward(xq_dqn* d, int which_net, const double* states_host, int n, double* q_host);
/* Same for n packed boards already in HBM ([n][12] u32): the one-hot of chessai.cpp:268-289 is never materialised.
 * q_dev: [n][ldq] fp32, first `n_out` outputs per row (n_out <= layer_sizes[last]). */
int xq_dqn_forward_boards_dev(xq_dqn* d, int which_net, const uint32_t* boards_dev, int n, int n_out,
                              float* q_dev, int ldq);
/* Q(s)[0..95] of the online net for n packed boards in HBM, through the SELECT chain of the self-play loop (what xq_trainer_collect
 * feeds the env kernel; DQN::selectAction reads q[action.to] only, dqn.cpp:47) -> q_dev [n][96] fp32.  Differs from
 * xq_dqn_forward_boards_dev(.., n_out = 96, ..) only in how it gets there: from 2048 boards on the head rides on the last hidden
 * product, and with xq_dqn_set_l0_derive the layer-0 sums of these boards are KEPT — while the online parameters do not change
 * (the plies of one update), the next call for the same board array derives them from the kept ones (rows of the squares that
 * changed out, rows of what stands there now in; boards more than 8 squares apart are summed in full). */
int xq_dqn_select_q_dev(xq_dqn* d, const uint32_t* boards_dev, int n, float* q_dev);
/* DQN::backpropagate(state, target, lr) / NeuralNetwork::backpropagate (dqn.cpp:59-62, dqn.cu:323-467) for a batch of
 * n (state, target) pairs: gradients of all n samples are taken at the pre-update weights, summed, scaled by
 * grad_scale and applied once (n = 1, grad_scale = 1 is exactly the upstream call).  mode = XQ_BACKPROP_*.  The reference's own
 * backpropagate(lr): plain SGD whatever xq_dqn_set_optimizer says, and it neither reads nor writes the optimizer state.
 * XQ_ERR_RUNTIME while a TD step waits for its apply_grads (between xq_dqn_td_grads* and xq_dqn_apply_grads under
 * xq_dqn_set_fused_apply(1)): its gradient sums use the workspaces that hold the waiting step's partial sums.  Nothing is uploaded or
 * launched then and no parameter moves.  xq_dqn_forward, xq_dqn_forward_boards_dev and xq_dqn_select_q_dev stay allowed in that window. */
int xq_dqn_backpropagate(xq_dqn* d, const double* states_host, const double* targets_host, int n,
                         double learning_rate, double grad_scale, int mode);
/* DQN::updateTargetNetwork() (dqn.cpp:71-73) — copies the TRAINED device weights (upstream copies stale host
 * vectors; documented divergence).  The optimizer state stays as it is. */
int xq_dqn_update_target(xq_dqn* d);
/* DQN::saveModel / loadModel (dqn.cpp:76-154): raw LE fp64 weights, raw fp64 biases, BE u64 count, BE i32 sizes.  The file holds no
 * optimizer state and loading leaves the handle's alone. */
int xq_dqn_save_model(xq_dqn* d, const char* path);
int xq_dqn_load_model(xq_dqn* d, const char* path);

/* The TD step of ChessAI::train (chessai.cpp:122-131) / DQN::train (dqn.cpp:157-172) on a batch of transitions held
 * in HBM:  y = done ? r : r + gamma * max_k Q_net(s')[k]  (max over ALL outputs);  target = Q(s) with entry
 * action.to replaced by y;  backprop of 0.5*|Q(s)-target|^2.  Split in two so a multi-GPU caller can all-reduce
 * the gradient buffer in between:
 *   xq_dqn_td_grads  : forward + deltas + gradient reduction over the batch  -> compact gradient buffer (HBM)
 *   xq_dqn_apply_grads: params -= lr * grad_scale * grads   (or the Adam step of xq_dqn_set_optimizer; clipped by xq_dqn_set_grad_clip)
 * boards/next_boards: [n][12] u32, optionally gathered through slots_dev ([n] row indices, NULL = identity).
 * td_net = XQ_TD_*.  loss_out_dev: optional, sum over the batch of 0.5*(Q(s,a)-y)^2 (of the Huber loss under xq_dqn_set_td_loss). */
int xq_dqn_td_grads(xq_dqn* d, const uint32_t* boards_dev, const uint32_t* next_boards_dev,
                    const int32_t* action_to_dev, const float* reward_dev, const uint8_t* done_dev,
                    const int32_t* slots_dev, int n, int td_net, int mode);
int xq_dqn_apply_grads(xq_dqn* d, double learning_rate, double grad_scale);
/* The flat gradient buffer xq_dqn_td_grads fills (fp32, *n_floats long) — what RCCL all-reduces over xGMI. */
int xq_dqn_grad_buffer(xq_dqn* d, float** grads_dev, size_t* n_floats);
/* on = 1: xq_dqn_apply_grads may sum the layer-0 gradient's partial sums itself (same order, bit-identical update, one
 * kernel fewer); the layer-0 segment of the gradient buffer is then NOT filled by xq_dqn_td_grads.  Leave 0 (default) when
 * anything reads the buffer between the two calls, e.g. a multi-GPU all-reduce. */
int xq_dqn_set_fused_apply(xq_dqn* d, int on);
/* The optimizer of xq_dqn_apply_grads (no upstream analogue: the reference knows p -= lr g only, dqn.cu:310-319).  XQ_OPT_SGD (default):
 * params -= lr * grad_scale * grads, the bits, kernels and launches of a handle that was never asked.  XQ_OPT_ADAM: torch.optim.Adam's
 * rule (amsgrad off, no weight decay) per touched parameter, at the t-th Adam apply since the state was last reset (t starts at 1):
 *   g' = grad_scale * g;  m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * with lr the learning_rate of xq_dqn_apply_grads, m, v, p in fp32, the two bias corrections computed on the host in double.  One
 * kernel in place of the SGD kernel (it sums pending partial sums itself in the same order, and refreshes the bf16 shadow); with a
 * communicator it runs behind the all-reduce, identically on every replica.  m and v cover exactly what the TD rule produces gradients
 * for (the layout of xq_dqn_grad_buffer); a parameter without a gradient keeps m = v = 0 and does not move, so output rows >= 96 stay
 * untouched as under SGD.  beta1 / beta2 / eps = 0 mean the defaults 0.9 / 0.999 / 1e-8; beta outside [0, 1), eps < 0 or an unknown kind
 * is XQ_ERR_INVALID_ARGUMENT; XQ_ERR_RUNTIME while a TD step waits for its apply_grads (as xq_dqn_set_fused_apply).  Changing the kind
 * zeroes m, v and t; a call that keeps the kind only replaces beta1 / beta2 / eps.  xq_dqn_set_params, xq_dqn_load_model and
 * xq_dqn_update_target leave the optimizer and its state alone; xq_dqn_backpropagate is always plain SGD. */
enum { XQ_OPT_SGD = 0, XQ_OPT_ADAM = 1 };
int xq_dqn_set_optimizer(xq_dqn* d, int kind, double beta1, double beta2, double eps);
/* Kind, the three constants in force and t (Adam applies since the last reset; 0 under SGD).  Any out pointer may be NULL. */
int xq_dqn_get_optimizer(const xq_dqn* d, int* kind, double* beta1, double* beta2, double* eps, uint64_t* steps);
/* m = v = 0 and t = 0, in order on the handle's stream; the kind and the constants stay.  A no-op under XQ_OPT_SGD. */
int xq_dqn_reset_optimizer(xq_dqn* d);
/* Adam's state to / from the host, for resuming a run and for tests: m and v in the layout of the gradient buffer (n_floats of
 * xq_dqn_grad_buffer each; get: either may be NULL), steps = t.  Both synchronise.  XQ_ERR_RUNTIME under XQ_OPT_SGD (no state). */
int xq_dqn_get_optimizer_state(xq_dqn* d, float* m_host, float* v_host, uint64_t* steps);
int xq_dqn_set_optimizer_state(xq_dqn* d, const float* m_host, const float* v_host, uint64_t steps);
/* Gradient clipping by the global L2 norm, in front of whatever optimizer xq_dqn_apply_grads runs (torch.nn.utils.clip_grad_norm_'s
 * rule; off by default, and a handle with it off runs the kernels, launches and bits of one that was never asked).  With g the summed
 * gradient about to be applied — every entry of the xq_dqn_grad_buffer layout, pending partial sums added in reduce_slabs_kernel's
 * order, behind an all-reduce the global sum:
 *   S    = sum_i (double)g_i^2                        every square and every sum in fp64, in one fixed association
 *   norm = |grad_scale| * sqrt(S)                     fp64: the norm of g' = grad_scale * g
 *   c    = (float) min(1, max_norm / (norm + 1e-6))
 *   SGD : p -= fl32(fl32(lr * grad_scale) * c) * g
 *   Adam: g' = fl32(fl32(grad_scale) * c) * g, then the element update of xq_dqn_set_optimizer unchanged
 * c == 1 makes both products exact: the update then has the bits of the unclipped one.  max_norm = +inf never clips and only measures
 * the norm.  A non-finite S gets no special case.  One kernel (grad_norm_kernel: fixed grid of 64 blocks per segment, so S does not
 * depend on the device or on whether the gradient arrived in slabs or in the buffer) in front of the apply kernel, which forms c itself
 * from the per-block partials: nothing returns to the host.  Side effect under xq_dqn_set_fused_apply: that kernel writes the slab sums
 * into the gradient buffer, which is therefore complete after the apply.  A gradient of 0 stays 0 (output rows >= 96 never move), the
 * bf16 shadow is refreshed as before, xq_dqn_backpropagate is never clipped.  The setting survives xq_dqn_set_optimizer,
 * xq_dqn_set_params, xq_dqn_load_model and xq_dqn_update_target.
 * 0 = off (default).  > 0 or +inf = on.  Negative or NaN: XQ_ERR_INVALID_ARGUMENT.  XQ_ERR_RUNTIME while a TD step waits for its
 * apply_grads. */
int xq_dqn_set_grad_clip(xq_dqn* d, double max_norm);
int xq_dqn_get_grad_clip(const xq_dqn* d, double* max_norm);
/* Of the last clipped-mode apply: its norm and coefficient.  Since clipping was last switched on (a change from 0): applies and how
 * many had c < 1.  Synchronises.  XQ_ERR_RUNTIME while off.  Any pointer may be NULL. */
int xq_dqn_grad_clip_stats(xq_dqn* d, double* last_norm, double* last_coef, uint64_t* applies, uint64_t* clipped);
/* Soft (Polyak) update of the target net, theta- <- theta- + tau (theta - theta-): extends DQN::updateTargetNetwork (dqn.cpp:71-74, a whole
 * copy) to the update a target-net user runs after every learn step.  Per parameter, with tau32 = (float)tau, p the online value and t the
 * target value:   d = fl32(p - t);   t' = fmaf(tau32, d, t)   (one rounding each; p == t leaves t' == t exactly).
 * xq_dqn_set_target_tau: tau in [0, 1], anything else or NaN is XQ_ERR_INVALID_ARGUMENT; XQ_ERR_RUNTIME while a TD step waits for its
 * apply_grads.  0 = off (default): the kernels, launches and bits of a handle that was never asked.  0 < tau < 1: every
 * xq_dqn_apply_grads moves the target net towards the online values it has just produced — SGD or Adam, clipped or not, from pending
 * partial sums or the gradient buffer, behind the all-reduce when a communicator is attached (identical on every replica).  While the
 * target's parameters outside what the TD rule touches have the online net's bits (after xq_dqn_create and xq_dqn_update_target) those
 * are fixed points and the update rides in the apply kernel itself over the touched segments: no further launch, the bf16 shadow of the
 * target follows.  After xq_dqn_set_params of either net, xq_dqn_load_model or xq_dqn_backpropagate one whole-buffer kernel follows the
 * apply instead, until the next xq_dqn_update_target; both forms give the same bits.  tau = 1 is the hard copy: xq_dqn_update_target
 * behind every apply (the element rule at 1 would not reproduce p where |t| >> |p|).  xq_dqn_backpropagate never touches the target.
 * The setting survives xq_dqn_set_optimizer, xq_dqn_set_grad_clip, xq_dqn_set_params, xq_dqn_load_model and xq_dqn_update_target. */
int xq_dqn_set_target_tau(xq_dqn* d, double tau);
int xq_dqn_get_target_tau(const xq_dqn* d, double* tau);
/* One soft update of the whole target net now, in order on the handle's stream, whatever xq_dqn_set_target_tau says (the facade's
 * updateTargetNetwork(tau), dqn.cpp:71-74 with a rate; a caller's own schedule).  tau = 1 is xq_dqn_update_target, tau = 0 a no-op, outside
 * [0, 1] or NaN XQ_ERR_INVALID_ARGUMENT. */
int xq_dqn_soft_update_target(xq_dqn* d, double tau);
/* The loss of the TD step (xq_dqn_td_grads*): the squared error (default; the bits, kernels and launches of a handle that was never asked)
 * or the error-clipped loss of Mnih et al. 2015 (Huber).  Per live sample (0 <= action.to < 96), with e = fl32(q - y), k = (float)kappa
 * and isw the importance weight of prioritized replay (1 otherwise):
 *   XQ_LOSS_SQUARED:  c = e                          loss = 0.5f e e
 *   XQ_LOSS_HUBER:    c = fminf(fmaxf(e, -k), k)     loss = |e| <= k ? 0.5f e e : k (|e| - 0.5f k)
 *   delta = c * (1 - q q) * isw
 * Only this scalar output delta changes: the hidden deltas, every gradient sum, both backprop modes, Adam, the clip, tau and the
 * all-reduce consume it as before; Double DQN and the bf16 nets take the same rule.  The importance weight multiplies behind the clamp,
 * and the priority written back stays (|e| + eps)^alpha of the RAW error, so what a run samples does not depend on kappa.  Where
 * |e| <= k, c has the bits of e: kappa above every |e| of a batch (+inf included) reproduces the squared loss bit for bit.
 * xq_dqn_last_loss (and the trainer's loss) carry the Huber loss while it is on; xq_dqn_backpropagate is never affected.
 * kappa > 0 or +inf for XQ_LOSS_HUBER (ignored for XQ_LOSS_SQUARED, which keeps the last one); an unknown kind, kappa <= 0, NaN or a kappa
 * that rounds to 0 as a float is XQ_ERR_INVALID_ARGUMENT; XQ_ERR_RUNTIME while a TD step waits for its apply_grads.  The setting survives
 * xq_dqn_set_optimizer, xq_dqn_set_grad_clip, xq_dqn_set_target_tau, xq_dqn_set_params, xq_dqn_load_model, xq_dqn_update_target and
 * xq_dqn_set_precision. */
enum { XQ_LOSS_SQUARED = 0, XQ_LOSS_HUBER = 1 };
int xq_dqn_set_td_loss(xq_dqn* d, int kind, double kappa);
int xq_dqn_get_td_loss(const xq_dqn* d, int* kind, double* kappa);
/* TD errors of the last xq_dqn_td_grads*, summarised on the device on request (one small kernel, off the step; synchronises): over the
 * live samples, with e = fl32(q - y) as the step formed it: their number, the mean of |e|, max |e|, the mean loss under the loss in force
 * (each sample's loss and both sums in fp64, one fixed association: the record does not depend on the device) and the number of samples
 * in the linear part, |e| > (float)kappa (0 under XQ_LOSS_SQUARED).  Means over 0 live samples are 0.  XQ_ERR_RUNTIME before the first
 * TD step.  Any out pointer may be NULL. */
int xq_dqn_td_error_stats(xq_dqn* d, uint64_t* live, double* mean_abs, double* max_abs, double* mean_loss, uint64_t* linear);
/* Convenience: sample-free TD update straight from a replay ring (slots from the last xq_replay_sample). */
int xq_dqn_td_grads_replay(xq_dqn* d, xq_replay* r, int batch, int td_net, int mode);
/* Host-buffer TD step for tests: n transitions as 90-byte boards. Returns Q(s,a) and y per sample if non-NULL. */
int xq_dqn_td_update_host(xq_dqn* d, int n, const uint8_t* boards90, const uint8_t* next_boards90,
                          const int32_t* action_to, const float* reward, const uint8_t* done, int td_net, int mode,
                          double learning_rate, double grad_scale, float* q_sa_out, float* y_out);
/* Sum-of-squared TD error of the last xq_dqn_td_grads, i.e. the sum of the per-sample loss in force (xq_dqn_set_td_loss; synchronises). */
int xq_dqn_last_loss(xq_dqn* d, double* loss);
/* Q(s,a) and the TD target y of the first n samples of the last xq_dqn_td_grads* (tests / interop; synchronises).  Either pointer
 * may be NULL. */
int xq_dqn_last_td_values(xq_dqn* d, int n, float* q_sa_host, float* y_host);
/* The first n rows of the batch the last xq_dqn_td_grads_replay assembled from a ring with n_step > 1 (xq_replay_set_n_step; tests /
 * interop; synchronises): the n-step reward R, done D, the number of chain elements used m, the sampled slot, the slot whose next board
 * was staged, and the staged action (-1: a dead row).  All outputs are host pointers, any of which may be NULL.  XQ_ERR_RUNTIME when
 * the last TD step was not an n-step one.  Behind a step that is both n-step and mirrored (xq_replay_set_mirror) `action` is the
 * mirrored one of the flagged rows; everything else is what it is without the mirror. */
int xq_dqn_last_n_step(xq_dqn* d, int n, float* reward, uint8_t* done, int32_t* steps, int32_t* first_slot, int32_t* last_slot,
                       int32_t* action);
/* The first n rows of the batch the last xq_dqn_td_grads_replay staged in mirror mode (xq_replay_set_mirror; tests / interop;
 * synchronises): the row's flag (1 = reflected), the two staged boards as 90 piece codes per row, the staged action and the sampled
 * slot.  All outputs are host pointers, any of which may be NULL.  XQ_ERR_RUNTIME when the last TD step was not a mirror-mode one,
 * XQ_ERR_INVALID_ARGUMENT for n beyond its rows. */
int xq_dqn_last_mirror(xq_dqn* d, int n, uint8_t* flags, uint8_t* boards90, uint8_t* next_boards90, int32_t* action_to, int32_t* slot);
/* The first n rows of the batch the last xq_dqn_td_grads_replay staged in colour-swap mode (xq_replay_set_colour_swap; tests / interop;
 * synchronises): the row's flag (1 = swapped), the two staged boards as 90 piece codes per row, the staged action, the staged side to
 * move in s' (next_player; only behind a step under the legal-move bootstrap, which is what stages it: asked for behind any other step
 * it is XQ_ERR_INVALID_ARGUMENT) and the sampled slot.  All outputs are host pointers, any of which may be NULL.  XQ_ERR_RUNTIME when
 * the last TD step was not a colour-swap-mode one, XQ_ERR_INVALID_ARGUMENT for n beyond its rows.  Behind a step with both symmetries on,
 * this call and xq_dqn_last_mirror report the same final staged batch (boards, action, slot: both transforms applied), each with its
 * own flags. */
int xq_dqn_last_colour_swap(xq_dqn* d, int n, uint8_t* flags, uint8_t* boards90, uint8_t* next_boards90, int32_t* action_to,
                            uint8_t* next_player /* optional */, int32_t* slot);
/* What the TD target bootstraps from (no upstream analogue: chessai.cpp:126 takes the maximum over all outputs).  XQ_BOOTSTRAP_ALL
 * (default): y = done ? r : r + gamma * max_k Q_net(s')[k] over ALL outputs — the kernels, launches and bits of a handle that was never
 * asked.  XQ_BOOTSTRAP_LEGAL: the maximum over the moves that can be played in s',
 *   y = done ? r : r + gamma * tanh(max over k of z(s')[to_k])
 * where (from_k, to_k) runs over getAllValidActions(s', side) in the canonical order (at most XQ_MAX_MOVES: a longer list is its first
 * 128), z is the output layer's pre-activation on the selecting net and the winner is chosen as everywhere (first maximum in list order,
 * a NaN never wins, nothing wins: entry 0 of the list) — the move xq_env_selfplay_step plays on the same values at epsilon 0.  A row whose
 * side has no move in s' takes y = r.  XQ_TD_ONLINE_NET / XQ_TD_TARGET_NET select and evaluate on one net; XQ_TD_DOUBLE selects on the
 * online net and takes the target net's pre-activation of the selected output.  The step then runs one 96-row product and one kernel
 * (legal_qmax_kernel: move generation, one wavefront per row) in place of the 8100-row maximum; xq_dqn_set_qmax_mode has no effect on
 * it (a legal step is never screened: the counters and the guard stand still), everything behind the target — loss, importance weights,
 * priorities, gradients, optimizers — is unchanged.
 * The side to move in s' cannot be recovered from (s, a, s') and is an input: xq_dqn_td_grads_sided / xq_dqn_td_update_host_sided take
 * it per transition (0 = Red, 1 = Black), and a replay ring records it once xq_replay_track_next_player was called: xq_dqn_td_grads_replay
 * then reads the ring's column — the sampled slot's byte; for an n-step batch the byte of the slot whose next board was staged; for a
 * mirrored batch the sampled slot's (a reflection does not change the side); one small gather (legal_side_stage_kernel) stages them; a
 * colour-swapped batch (xq_replay_set_colour_swap) has them staged by its own kernel, 1 - side on the flagged rows.
 * While XQ_BOOTSTRAP_LEGAL is in force the step is XQ_ERR_INVALID_ARGUMENT through every entry that has no side — xq_dqn_td_grads,
 * xq_dqn_td_update_host, xq_dqn_td_grads_replay from a ring that does not track it — and on a bf16 precision (fp32 nets only).  An unknown kind, or XQ_BOOTSTRAP_LEGAL on a net with fewer than 96 outputs, is
 * XQ_ERR_INVALID_ARGUMENT.  The setting may change between any two steps and survives every other setter. */
enum { XQ_BOOTSTRAP_ALL = 0, XQ_BOOTSTRAP_LEGAL = 1 };
int xq_dqn_set_td_bootstrap(xq_dqn* d, int kind);
int xq_dqn_get_td_bootstrap(const xq_dqn* d, int* kind);
/* xq_dqn_td_grads with the side to move in each next board: next_player_dev is [rows] u8 (0 = Red, 1 = Black; not validated on the
 * device, where any non-zero byte is taken as Black), read through
 * slots_dev like done_dev.  Under XQ_BOOTSTRAP_ALL the side bytes are not read and the step is xq_dqn_td_grads.  Boards must satisfy
 * what xq_env_set_state asks (piece codes <= 14, at most 16 pieces of one colour). */
int xq_dqn_td_grads_sided(xq_dqn* d, const uint32_t* boards_dev, const uint32_t* next_boards_dev, const int32_t* action_to_dev,
                          const float* reward_dev, const uint8_t* done_dev, const uint8_t* next_player_dev, const int32_t* slots_dev,
                          int n, int td_net, int mode);
/* xq_dqn_td_update_host with next_player[n] (0 or 1; anything else, or a next board with more than 16 pieces of one colour, is
 * XQ_ERR_INVALID_ARGUMENT). */
int xq_dqn_td_update_host_sided(xq_dqn* d, int n, const uint8_t* boards90, const uint8_t* next_boards90, const int32_t* action_to,
                                const float* reward, const uint8_t* done, const uint8_t* next_player, int td_net, int mode,
                                double learning_rate, double grad_scale, float* q_sa_out, float* y_out);
/* The first n rows of the last TD step if it ran under XQ_BOOTSTRAP_LEGAL (tests / interop; synchronises): the length of the row's move
 * list (0: no move; -1: a done row or a dead one, action < 0, for which no list was generated), the winning `to` (-1 where there is no
 * winner), the pre-activation the target took (0 where y = r) and, optionally, the selecting net's 96 pre-activations per row, [n][96].
 * All outputs are host pointers, any of which may be NULL.  XQ_ERR_RUNTIME when the last TD step was not a legal one,
 * XQ_ERR_INVALID_ARGUMENT for n beyond its rows. */
int xq_dqn_last_legal(xq_dqn* d, int n, int32_t* n_moves, int32_t* a_star, float* zmax, float* z96);
/* The zero-sum (negamax) target for self-play (DESIGN.md §4 "Zero-sum target"; no upstream analogue).  on = 0 (default): every handle,
 * launch and bit is what it is without this call.  on = 1: s' of a self-play transition has the OTHER side to move, so its best value
 * counts against the mover of s.  With g = (float)gamma,
 *   y = done ? r : r - g * tanh(zm)
 * where zm is exactly what it is for the handle's bootstrap, td_net and precision (the screened or exact maximum over all outputs, or
 * the legal-move maximum, Double DQN's evaluation on the target net).  The step's kernels are the same: they take the signed discount
 * -g through the argument they have (r + (-g) t and r - g t are the same fp32 bits).  Loss, importance weights, priorities
 * (|q - y| + eps)^alpha and xq_dqn_td_error_stats follow the new y and are otherwise unchanged.
 * n-step batches (xq_replay_set_n_step): disc_0 = 1, disc_k = fl32(disc_{k-1} * (-g)) — today's magnitudes with the sign (-1)^k — and
 * the step's discount is disc_n: in a self-play ring the chain's slots alternate movers, so this is the negamax n-step return.
 * Under XQ_BOOTSTRAP_LEGAL a row whose side to move in s' has no move bootstraps from -inf (xq_dqn_last_legal: zmax = -inf, a_star = -1,
 * n_moves = 0): tanh(-inf) = -1 is the lowest value the net can express, a side that cannot move has lost, y = r + g.  Done and dead
 * rows keep zmax = 0.
 * Applies to xq_dqn_td_grads, _sided, _replay (n-step, mirrored and colour-swapped batches too), xq_dqn_td_update_host and _sided; not
 * to xq_dqn_backpropagate (the caller's targets).  on other than 0 or 1: XQ_ERR_INVALID_ARGUMENT; XQ_ERR_RUNTIME while a TD step waits
 * for its apply_grads.  The setting survives every other setter, xq_dqn_set_params, xq_dqn_load_model and xq_dqn_update_target.
 * The net still sees absolute colours and no side to move; a ring holding rows from before a switch gets the current sign on all of
 * them. */
int xq_dqn_set_zero_sum(xq_dqn* d, int on);
int xq_dqn_get_zero_sum(const xq_dqn* d, int* on);
/* The ring's side-to-move column (for XQ_BOOTSTRAP_LEGAL): one byte per slot, the side to move in the stored next board.  The column is
 * allocated by xq_replay_track_next_player, which must come while the ring is empty (XQ_ERR_RUNTIME otherwise; a second call is a
 * no-op); a ring that never tracked is the ring of before, array for array.  On a tracking ring every transition written by
 * xq_env_selfplay_step carries 1 - mover, every one written by versus training the learner's colour; xq_replay_push_host is
 * XQ_ERR_INVALID_ARGUMENT and xq_replay_push_host_sided pushes with next_player[n] (0 or 1).  xq_replay_get_next_player copies slots
 * [first, first + n) to the host (tests; synchronises; XQ_ERR_RUNTIME on a ring that does not track).  The column belongs to
 * XQ_ORDER_RING_CONTENTS. */
int xq_replay_track_next_player(xq_replay* r);
int xq_replay_push_host_sided(xq_replay* r, int n, const uint8_t* boards90, const int32_t* action_to, const float* reward,
                              const uint8_t* done, const uint8_t* next_boards90, const uint8_t* next_player);
int xq_replay_get_next_player(xq_replay* r, int first, int n, uint8_t* out);
/* Mover view (DESIGN.md §4 "Mover view").  Write swap for the colour-swap map: board'[(9 - r) 9 + c] = sigma(board[r 9 + c]) and
 * a' = a + 81 - 18 (a div 9) for 0 <= a < 90, any other value as it is.  view(board, side) is board when side == 0 (Red) and
 * swap(board) when side == 1.  A net with XQ_VIEW_MOVER reads view(s, side to move in s), and its output k is the value of moving to
 * square k OF THE VIEW: on an absolute board with Black to move the value of the destination `to` is output swap(to).  A transition
 * (s, a, r, s', done) with mover m and next side p trains on (view(s, m), m ? swap(a) : a, r, view(s', p), done); in that batch the side
 * to move in s' is always Red.  Reward, done, discounts, zero-sum, the loss, n-step, mirror and prioritized replay do not change; the ring
 * keeps absolute boards and absolute action_to.
 * The view is a property of the handle, XQ_VIEW_ABSOLUTE by default: unknown values are XQ_ERR_INVALID_ARGUMENT, a change while a TD step
 * waits for its apply_grads is XQ_ERR_RUNTIME, and it survives every other setter, xq_dqn_set_params, xq_dqn_load_model and
 * xq_dqn_update_target.  It is not stored in the model file.
 * The paths that know the side honour it: xq_dqn_td_grads_replay (below) and an env told that its rows are in the view
 * (xq_env_set_q_view).  The raw-pointer and host entry points — xq_dqn_td_grads, _sided, xq_dqn_td_update_host*, xq_dqn_forward*,
 * xq_dqn_select_q_dev, xq_dqn_backpropagate — take boards AS THE NET READS THEM and transform nothing: a caller who wants the view
 * builds it with xq_view_boards_dev.
 * xq_dqn_td_grads_replay under XQ_VIEW_MOVER stages the minibatch with one more kernel, mover_view_stage_kernel, the last staging
 * transform (n-step, then mirror, then view): s and the action by mover[first slot], s' by next_player[the slot whose s' was staged],
 * and under XQ_BOOTSTRAP_LEGAL the staged side byte 0 on every row.  The step then runs on the staged batch unchanged, a prioritized
 * draw's priorities go to the sampled slots.  XQ_ERR_INVALID_ARGUMENT from a ring that does not track both columns
 * (xq_replay_track_mover, xq_replay_track_next_player), and from a ring with xq_replay_set_colour_swap(prob > 0): the view of a swapped
 * transition is the view of the transition bit for bit, so the augmentation would only spend a launch. */
enum { XQ_VIEW_ABSOLUTE = 0, XQ_VIEW_MOVER = 1 };
int xq_dqn_set_view(xq_dqn* d, int view);
int xq_dqn_get_view(const xq_dqn* d, int* view);
/* out_dev[b] = view(boards_dev[b], side_dev[b]) for n packed boards (12 words each; side_dev: [n] u8, 0 = Red, anything else Black),
 * queued on hip_stream (nullptr: the default stream).  out_dev must not be boards_dev.  Nibbles 90..95 of a swapped board come out 0. */
int xq_view_boards_dev(const void* boards_dev, const void* side_dev, int n, void* out_dev, void* hip_stream);
/* The first n rows of the batch the last xq_dqn_td_grads_replay staged under XQ_VIEW_MOVER (tests / interop; XQ_ERR_RUNTIME if the last
 * TD step was not a view-mode one): the two flags per row, the staged boards (90 piece codes each), actions and sampled slots.  Every
 * pointer is optional.  Synchronises the handle's stream. */
int xq_dqn_last_view(xq_dqn* d, int n, uint8_t* flag_s, uint8_t* flag_next, uint8_t* boards90, uint8_t* next_boards90, int32_t* action_to,
                     int32_t* slot);
/* The ring's who-moved column (for XQ_VIEW_MOVER): one byte per slot, the side that moved in the stored board — in versus training the
 * learner's colour, which (s, a.to, s') does not tell.  next_player's sibling, by the same rules: xq_replay_track_mover allocates it
 * while the ring is empty (XQ_ERR_RUNTIME otherwise; a second call is a no-op); on a tracking ring every transition written by
 * xq_env_selfplay_step carries its mover and every one written by versus training the learner's colour; xq_replay_push_host and
 * xq_replay_push_host_sided are XQ_ERR_INVALID_ARGUMENT and xq_replay_push_host_sides pushes with mover[n] and, exactly if the ring
 * tracks that column too, next_player[n] (else nullptr).  xq_replay_get_mover copies slots [first, first + n) to the host (tests;
 * synchronises; XQ_ERR_RUNTIME on a ring that does not track).  The column belongs to XQ_ORDER_RING_CONTENTS. */
int xq_replay_track_mover(xq_replay* r);
int xq_replay_push_host_sides(xq_replay* r, int n, const uint8_t* boards90, const int32_t* action_to, const float* reward,
                              const uint8_t* done, const uint8_t* next_boards90, const uint8_t* mover, const uint8_t* next_player);
int xq_replay_get_mover(xq_replay* r, int first, int n, uint8_t* out);
/* "The Q rows handed to xq_env_selfplay_step* are in the mover's view": where the greedy pick reads q[to] it reads q[swap(to)] when
 * Black is to move.  Nothing else of the step changes; the ring's action_to stays absolute.  Exact ties may resolve to another move than
 * on the absolute board with permuted rows would, only in that the scan order of the move list is not symmetric: the pick is the first
 * maximum over the list in its own order either way.  on other than 0 or 1: XQ_ERR_INVALID_ARGUMENT. */
int xq_env_set_q_view(xq_env* e, int on);
int xq_env_get_q_view(const xq_env* e, int* on);
/* Per-kernel HIP-event timing on the handle stream, for bench.py (name -> summed ms, launches, algorithmic flops/bytes).
 * enable: -1 leave, 0 off, 1 on, 2 on + clear, 3 on + clear but bracket only the TD step's dominant GEMM (gemm_qmax_rowmax /
 * gemm_qmax_screen) and env_selfplay_step, 4 = 3 with the GEMM bracketed on every 4th launch only (a pair of event records
 * drains the stream's queue: ~10 us per bracket). */
/* exact_launches: how many of `launches` were timed by the kernel's OWN start / stop events (single-kernel brackets, launched with
 * hipExtLaunchKernelGGL): their ms is the kernel's duration as a profiler reports it; the others are pairs of recorded events around the
 * launch(es), which read ~6.5 us more per bracket. */
typedef struct { char name[48]; float ms; int launches; double flops; double bytes; int exact_launches; int reserved; } xq_kernel_stat;
int xq_dqn_kernel_stats(xq_dqn* d, int enable, xq_kernel_stat* stats, int max_stats, int* n_stats);
/* Which launches enable = 3 / 4 bracket: a comma-separated list of bracket names as xq_dqn_kernel_stats reports them (launches of the
 * self-play loop's select chain on the trainer's collect stream carry the suffix "@select"; "rccl_allreduce_grads" = the gradient
 * all-reduce of a data-parallel step).  NULL / "" = the default: gemm_qmax_rowmax, gemm_qmax_screen, env_selfplay_step.  bench.py
 * walks the kernels of the step with it one at a time (roofline_chain), so that each is measured with only its own bracket in the loop. */
int xq_dqn_kernel_filter(xq_dqn* d, const char* names_csv);
/* Live timeline of the brackets gathered by the last xq_dqn_kernel_stats call (enable 1/2 sessions): start/end of every
 * bracketed launch in ms relative to the first one, across the handle's streams — what a kernel trace shows, without a
 * profiler attached.  Diagnostic. */
typedef struct { char name[48]; float start_ms; float end_ms; } xq_kernel_span;
int xq_dqn_kernel_timeline(xq_dqn* d, xq_kernel_span* spans, int max_spans, int* n_spans);

/* ------------------------------------------------------------------------------------------------------------
 * xq_comm — the one exchange step of the data-parallel loop (no upstream analogue: the reference is
 * single-GPU): games are sharded over ranks by contiguous game-id ranges, one process per GPU, and each update sums
 * the compact TD gradient buffer over all ranks with an RCCL all-reduce over xGMI; every replica then applies the same SGD
 * step (xq_trainer_learn_apply scales by 1/(minibatch*world)).  RCCL is loaded on first use.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct xq_comm xq_comm;
enum { XQ_COMM_ID_BYTES = 128 };
/* rank 0 draws the communicator id (ncclGetUniqueId) and ships the 128 bytes to the other ranks out of band. */
int xq_comm_unique_id(uint8_t* id128);
/* ncclCommInitRank on the calling process's current device (xq_set_device).  Collective: every rank calls it. */
int xq_comm_create(int rank, int world, const uint8_t* id128, xq_comm** out);
/* Same, with the id exchanged through a file every rank can see (rank 0 writes, the others poll up to timeout_s).  `path` must
 * not exist beforehand (rank 0 refuses a leftover, XQ_ERR_IO: it would hand the other ranks a dead id); rank 0 removes the file
 * again once every rank has joined, so one path serves run after run. */
int xq_comm_create_from_file(int rank, int world, const char* path, double timeout_s, xq_comm** out);
int xq_comm_destroy(xq_comm* c);
int xq_comm_info(const xq_comm* c, int* rank, int* world, uint64_t* collectives_issued, uint64_t* floats_reduced);
/* Sum of one host counter over all ranks (blocking; control decisions every rank must take alike, e.g. "enough episodes"). */
int xq_comm_sum_u64(xq_comm* c, uint64_t* inout_host);
/* In-place sum of n_floats fp32 over all ranks on hip_stream (NULL = the communicator's own stream). */
int xq_comm_allreduce(xq_comm* c, float* buf_dev, size_t n_floats, void* hip_stream);
/* Attach (or detach with NULL) a communicator: every xq_dqn_td_grads* then all-reduces the gradient buffer itself, on the stream of
 * its producer right behind it (no communicator stream, no extra events).  fp32 nets (fused launches, xq_dqn_set_td_tail): ONE
 * collective over the whole buffer on the handle's stream, behind the launch that reduces the step's partial sums into it.  bf16
 * nets and xq_dqn_set_td_tail(0): two buckets — [hidden + output-layer weights, biases] on the library's side stream, issued first,
 * the layer-0 segment (the largest and last) on the handle's stream behind the layer-0 kernel.  Either way the call returns with
 * the handle's stream ordered behind the exchange; xq_dqn_apply_grads therefore sees the global sum.  world = 1 is bit-identical
 * to no communicator. */
int xq_dqn_set_comm(xq_dqn* d, xq_comm* comm);
/* Where the event the trainer's select chain waits for is recorded in a data-parallel TD step (fp32 nets, fused launches).  0: behind
 * the max pass, as on one GPU (the select chain runs beside the gradient kernels; the all-reduce is exposed).  1: behind the gradient
 * kernels, in front of the all-reduce (the select chain runs beside the exchange and hides it; costs ~41 us of overlap with the
 * gradient kernels).  -1 (default): decided by MEASUREMENT — xq_dqn_set_comm with a communicator of more than one rank times 20
 * all-reduces of the gradient buffer (xq_dqn_calibrate_exchange) and takes 1 iff their mean exceeds 41 us; one rank: 0.  No effect
 * without a communicator.  Same results either way. */
int xq_dqn_set_exchange_overlap(xq_dqn* d, int mode);
/* COLLECTIVE (every rank of the attached communicator, same point of the program): times 4 + 20 all-reduces of a scratch buffer of the
 * gradient buffer's size on the handle's stream, averages the mean over the ranks and sets the -1 (auto) choice above to "late" iff
 * it exceeds threshold_us (< 0: the library's 41 us).  Works with one rank too (tests force both branches with the threshold).
 * xq_dqn_exchange_calibration reads back what the last calibration measured and chose (calibrated = 0: none yet). */
int xq_dqn_calibrate_exchange(xq_dqn* d, double threshold_us, double* allreduce_us, int* late);
int xq_dqn_exchange_calibration(const xq_dqn* d, int* calibrated, double* allreduce_us, double* threshold_us, int* late);
/* One all-reduce of the whole gradient buffer on the handle's stream, for callers that do not attach a communicator. */
int xq_allreduce_grads(xq_dqn* d, xq_comm* comm);

/* ------------------------------------------------------------------------------------------------------------
 * xq_arena — playing strength: player A against player B over n_pairs PAIRS of games, all 2 n_pairs games at once
 * (no upstream analogue beyond ChessAI::getAIMove, chessai.cpp:29-83, one game and one net at a time; DESIGN.md §4 "Arena").
 *   seats    : games [0, n_pairs) have A as Red, games [n_pairs, 2 n_pairs) have A as Black; game g and g + n_pairs are twins;
 *   opening  : the first opening_plies plies are uniform-random on the PAIR's Philox stream (ctr = {ply, 0, first_game_id + g mod
 *              n_pairs, 0}), so twins play the same opening with the seats swapped; then game g draws on its own id first_game_id + g;
 *   moves    : each player moves like xq_env_selfplay_step (epsilon-greedy over q[action.to] of the legal list, first maximum wins,
 *              same Philox draws) with an epsilon of its own; a NULL player always takes the uniform-random branch.  First maximum,
 *              for non-finite values too (dqn.cpp:39-51: maxQ = -inf, bestAction = validActions[0], strict >): of equal maxima the
 *              first list entry wins, +0 equals -0, denormals compare by value, +inf wins like any value, a NaN never wins, and a
 *              row whose candidates are all NaN or -inf plays validActions[0];
 *   end      : a game stops on the ply that ends it (a general captured, no legal action for the side to move, the 200-move cap,
 *              chessboard.cpp:286-309) and stays frozen — no reset, no replay write — with its record written on that ply.
 * A player handle is borrowed: the arena runs its forwards through xq_dqn_forward_boards_dev on the handle's stream (no kept
 * layer-0 sums, no TD-step state, no kernel statistics), so a training run that lends its network gets the same bits afterwards.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct xq_arena xq_arena;
enum {
    XQ_ARENA_LIVE = 0,              /* still playing */
    XQ_ARENA_GENERAL_CAPTURED = 1,  /* the side that captured the general wins */
    XQ_ARENA_NO_LEGAL_MOVE = 2,     /* build-defined: the side to move with no legal action loses (upstream just ends the episode) */
    XQ_ARENA_MOVE_CAP = 3,          /* the 200-move cap: a draw here (getWinner() says Red, which would reward the Red seat) */
    XQ_ARENA_OPENING = 4            /* ended inside the random opening: reported, never scored (its twin ended the same way) */
};
typedef struct {
    uint8_t cause;                  /* XQ_ARENA_* */
    uint8_t winner;                 /* getWinner() on the final board (chessboard.cpp:312-320), 2 while live */
    int8_t a_result;                /* +1 A won, 0 draw / opening / live, -1 A lost */
    uint8_t a_is_red;
    uint16_t plies;                 /* getMoveCount() of the final board */
    int16_t red_score, black_score; /* getRedScore() / getBlackScore() of the final board */
    uint16_t reserved;
} xq_arena_game;
/* n_pairs > 0 pairs (2 n_pairs games, one xq_env of its own on hip_stream, NULL = its own stream); seed and first_game_id key the
 * Philox streams as for xq_env_create.  The arena starts reset with the default opening of 8 plies. */
int xq_arena_create(int n_pairs, uint64_t seed, uint32_t first_game_id, void* hip_stream, xq_arena** out);
int xq_arena_destroy(xq_arena* a);
/* Every game back to the start position, every record live, 0 <= opening_plies <= 200 random plies to come. */
int xq_arena_reset(xq_arena* a, int opening_plies);
/* One ply with caller-supplied Q rows: q_dev = [2 n_pairs] rows of q_stride >= 90 floats (tanh Q of outputs 0..89) on the arena's
 * device, ordered behind the arena's stream by the caller (NULL = both players random); eps_a / eps_b in [0, 1] are the players'
 * epsilons.  A's rows are read from the half where A is to move.  INVALID_ARGUMENT once no game is live. */
int xq_arena_ply_q_dev(xq_arena* a, const float* q_dev, int q_stride, double eps_a, double eps_b);
/* ... with a flag per player (0 or 1): that player's rows are in the mover's view (DESIGN.md §4 "Mover view"; the caller computed them on
 * xq_view_boards_dev's boards), so where it moves as Black the pick reads q[swap(to)].  (0, 0) is xq_arena_ply_q_dev.  A network player
 * of xq_arena_run / xq_arena_run_players is read through its own handle's view (xq_dqn_set_view) without further ado. */
int xq_arena_ply_q_dev_view(xq_arena* a, const float* q_dev, int q_stride, double eps_a, double eps_b, int view_a, int view_b);
/* A Boltzmann temperature per player (xq_env_set_policy's rule on that player's non-epsilon plies), 0 = greedy, else as fp32 finite and
 * in [1e-3, 1e3]; anything else is XQ_ERR_INVALID_ARGUMENT and nothing changes.  Honoured for XQ_PLAYER_NET players and for
 * caller-supplied rows (xq_arena_ply_q_dev*, xq_arena_run, xq_arena_run_players) from the next ply on; ignored for random and search
 * players and in the opening.  Survives xq_arena_reset.  After the opening twins draw on their own game ids, as the epsilon draws do.
 * xq_arena_get_temperature: the values as last given, (0, 0) on an arena that was never asked.  Outputs may be NULL. */
int xq_arena_set_temperature(xq_arena* a, double temp_a, double temp_b);
int xq_arena_get_temperature(const xq_arena* a, double* temp_a, double* temp_b);
/* Plays until no game is live or max_plies plies (<= 0: no limit) have been played by this call; *plies_played (optional) = how many.
 * dqn_a / dqn_b: a network with layer_sizes[0] == 1260 and >= 90 outputs, or NULL for uniform-random play; dqn_a == dqn_b is allowed,
 * and so are handles on different streams (ordered by events).  eps_a, eps_b in [0, 1]. */
int xq_arena_run(xq_arena* a, xq_dqn* dqn_a, xq_dqn* dqn_b, double eps_a, double eps_b, int max_plies, int* plies_played);
/* A player of xq_arena_run_players.  kind XQ_PLAYER_RANDOM: uniform-random play (dqn, depth, eps unused); XQ_PLAYER_NET: the borrowed
 * network dqn (as for xq_arena_run) with exploration eps; XQ_PLAYER_SEARCH: the material search of xq_env_search at depth 1..3 with
 * exploration eps — greedy plies take one of the best root moves, ties broken uniformly on the PAIR's Philox stream (ctr = {ply, 0,
 * first_game_id + g mod n_pairs, 3}), so twins break ties alike and a search player against itself at eps = 0 scores exactly 0.5. */
enum { XQ_PLAYER_RANDOM = 0, XQ_PLAYER_NET = 1, XQ_PLAYER_SEARCH = 2 };
typedef struct {
    int kind;                       /* XQ_PLAYER_* */
    xq_dqn* dqn;                    /* XQ_PLAYER_NET: the network (layer_sizes[0] == 1260, >= 90 outputs) */
    int depth;                      /* XQ_PLAYER_SEARCH: 1, 2 or 3 */
    double eps;                     /* XQ_PLAYER_NET / XQ_PLAYER_SEARCH: exploration in [0, 1] */
} xq_arena_player;
/* xq_arena_run with any two players (NULL = XQ_PLAYER_RANDOM).  An invalid kind, depth or eps, or a NULL dqn for XQ_PLAYER_NET:
 * INVALID_ARGUMENT.  The search runs on the arena's stream, one launch per ply and searching half, over the live games only. */
int xq_arena_run_players(xq_arena* a, const xq_arena_player* pa, const xq_arena_player* pb, int max_plies, int* plies_played);
/* [2 n_pairs] records (live games report their current plies and scores). */
int xq_arena_results(xq_arena* a, xq_arena_game* records_host);
int xq_arena_live(xq_arena* a, int* n_live);
int xq_arena_env(xq_arena* a, xq_env** env);                 /* the arena's games (get_state etc.); owned by the arena */
/* The per-game xq_step_result of the last ply (a move trace for tests); defined for the games that were live before that ply. */
int xq_arena_last_step(xq_arena* a, xq_step_result* results_host);

/* ------------------------------------------------------------------------------------------------------------
 * xq_trainer — the ChessAI::train() loop (chessai.cpp:85-170) for n_games boards at once, on device.
 *   collect : Q(s)[0..89] for every game -> xq_env_selfplay_step -> transitions into the replay ring
 *   learn   : sample minibatch -> xq_dqn_td_grads  [caller may all-reduce xq_dqn_grad_buffer] -> apply
 *   target sync every target_sync_interval learn steps (chessai.cpp:140 uses moveCount % 100).
 * With overlap_collect the same three calls are issued in the same order; collect is queued on a second stream and
 * learn_apply joins it, so env stepping hides behind the TD step (and behind the caller's gradient all-reduce).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct xq_trainer xq_trainer;
typedef struct {
    int n_games;
    int layer_sizes[XQ_MAX_LAYERS + 1];
    int n_sizes;
    double learning_rate, gamma, epsilon;   /* chessai.h:48-49, chessai.cpp:106 */
    int replay_capacity;                    /* 0 => on-policy: learn on the n_games transitions just collected (reference semantics) */
    int minibatch;                          /* transitions per learn step (<= replay capacity; on-policy: n_games) */
    int td_net;                             /* XQ_TD_* */
    int backprop_mode;                      /* XQ_BACKPROP_* */
    int target_sync_interval;               /* learn steps between updateTargetNetwork(); 0 = never */
    int mean_gradient;                      /* 1: grad_scale = 1/(minibatch*world), 0: sum (grad_scale = 1) */
    uint64_t seed;
    uint32_t first_game_id;
    int collects_per_update;                /* plies played in every game per learn step (0 or 1 = one; BASELINE configs[3] uses 4) */
    int overlap_collect;                    /* 1: collect runs on its own HIP stream beside learn_grads of the same iteration; both
                                             * read the same parameters, and the minibatch is drawn from the ring minus the slots the
                                             * collect is writing (they become eligible one iteration later).  Needs a replay ring. */
    /* build-defined modes of BASELINE configs[4] (td_net = XQ_TD_DOUBLE selects Double DQN): */
    int prioritized;                        /* 1: proportional prioritized replay (xq_replay_enable_per); the minibatch never contains
                                             * the slots this iteration's collects write: they are retired from the tree at learn_apply */
    double per_alpha, per_beta, per_eps;    /* 0 => 0.6, 0.4, 1e-3 */
    int precision;                          /* XQ_PRECISION_* of the Q-network's forward passes */
} xq_trainer_config;

int xq_trainer_create(const xq_trainer_config* cfg, void* hip_stream, xq_trainer** out);
int xq_trainer_destroy(xq_trainer* t);
int xq_trainer_env(xq_trainer* t, xq_env** env);
/* The trainer's network (borrowed).  Its optimizer is chosen here: xq_dqn_set_optimizer(dqn, ...) between iterations; learn_apply
 * passes cfg.learning_rate and the gradient scale to xq_dqn_apply_grads whatever the kind. */
int xq_trainer_dqn(xq_trainer* t, xq_dqn** dqn);
int xq_trainer_replay(xq_trainer* t, xq_replay** replay);
/* xq_dqn_set_comm on the trainer's network: learn_grads then carries the bucketed all-reduce, learn_apply(world) the mean. */
int xq_trainer_set_comm(xq_trainer* t, xq_comm* comm);
/* n_plies uniform-random plies in every game (no Q-network, nothing written to the replay ring, not counted as env steps):
 * desynchronises the games so that a measurement or a training run starts from a spread of game phases rather than from
 * n_games copies of the opening.  Call between iterations. */
int xq_trainer_random_plies(xq_trainer* t, int n_plies);
/* Which rule gives the TD target from the next learn step on: XQ_TD_ONLINE_NET (ChessAI::train, chessai.cpp:126), XQ_TD_TARGET_NET
 * (DQN::train, dqn.cpp:166) or XQ_TD_DOUBLE.  Call between iterations. */
int xq_trainer_set_td_net(xq_trainer* t, int td_net);
/* xq_dqn_set_target_tau on the trainer's network (DQN::updateTargetNetwork, dqn.cpp:71-74, as a soft update inside every learn_apply).
 * target_sync_interval keeps its meaning: a user of tau sets it to 0; if both are set, both happen.  Call between iterations. */
int xq_trainer_set_target_tau(xq_trainer* t, double tau);
/* xq_replay_set_n_step(ring, n, n_games) on the trainer's ring, and the windows that go with it (DESIGN.md §4 "n-step returns").
 * Uniform replay: the minibatch is drawn from the oldest readable slot on, without the slots in flight (as always) and without the
 * newest (n - 1) * n_games slots in front of them, whose chains are not complete; the chains read the window before that last cut.  If
 * the cut would leave nothing (the first iterations of a run) the uncut window is sampled and the rows that reach past it are dead.
 * Prioritized replay: both rebuilds hold the newest (n - 1) * n_games slots (xq_replay_per_rebuild_hold); the chains read the filled
 * ring minus the slots about to be retired.  Self-play and versus training, any collects_per_update, with and without overlap_collect.
 * n > 1 needs a replay ring whose capacity exceeds (n - 1 + collects_per_update) * n_games: otherwise, or on-policy, it is
 * XQ_ERR_INVALID_ARGUMENT.  Call between iterations. */
int xq_trainer_set_n_step(xq_trainer* t, int n_step);
/* xq_replay_set_mirror on the trainer's ring (DESIGN.md §4 "Mirror augmentation"): every learn_grads from then on mirrors a random
 * part of its minibatch — uniform and prioritized replay, on-policy too (the identity batch), with and without overlap_collect, with
 * any n_step.  No window changes: the transform reads only what the step read anyway.  Call between iterations: XQ_ERR_RUNTIME while a
 * learn_grads waits for its learn_apply. */
int xq_trainer_set_mirror(xq_trainer* t, double prob);
/* xq_replay_set_colour_swap on the trainer's ring (DESIGN.md §4 "Colour-swap augmentation"): every learn_grads from then on exchanges
 * the colours of a random part of its minibatch — uniform, prioritized and on-policy rings, any n_step, overlap_collect 0 and 1,
 * self-play and versus, with or without the mirror and under both bootstraps.  No window changes.  Call between iterations:
 * XQ_ERR_RUNTIME while a learn_grads waits for its learn_apply. */
int xq_trainer_set_colour_swap(xq_trainer* t, double prob);
/* xq_env_set_reward on the trainer's env (DESIGN.md §4 "Reward rule"): the next collect writes the new reward, slots already in the ring
 * keep theirs.  Uniform, prioritized and on-policy rings, overlap_collect 0 and 1, self-play and versus; n-step returns, the mirror,
 * prioritized replay and both bootstraps read the ring's reward column as before.  Call between iterations: XQ_ERR_RUNTIME while a
 * learn_grads waits for its learn_apply. */
int xq_trainer_set_reward(xq_trainer* t, int kind, double scale, double ply_cost, double bound);
/* xq_env_set_policy on the trainer's env (DESIGN.md §4 "Exploration policy"): the next collect queued picks by it.  Self-play and the
 * learner of versus training (the opponent stays epsilon-greedy), uniform, prioritized and on-policy rings, overlap_collect 0 and 1. */
int xq_trainer_set_policy(xq_trainer* t, int kind, double temperature);
/* The exploration rate of the collects (xq_trainer_config.epsilon), 0 <= eps <= 1; a NaN or a value outside: XQ_ERR_INVALID_ARGUMENT and
 * nothing changes.  Legal between any two collects, with overlap_collect too: the next collect queued reads the new value, one already
 * queued keeps the value it was launched with.  Versus training: the learner's epsilon; the opponent's stays its own. */
int xq_trainer_set_epsilon(xq_trainer* t, double eps);
int xq_trainer_get_epsilon(const xq_trainer* t, double* eps);
/* xq_dqn_set_td_bootstrap on the trainer's Q-net.  XQ_BOOTSTRAP_LEGAL first turns tracking on for the trainer's ring, so call it before
 * the first collect: XQ_ERR_RUNTIME once the ring holds a transition (unless it tracks already).  Back to XQ_BOOTSTRAP_ALL is allowed
 * between iterations (XQ_ERR_RUNTIME while a learn_grads waits for its learn_apply); the column keeps being written.  Uniform,
 * prioritized and on-policy rings, overlap_collect 0 and 1, self-play and versus. */
int xq_trainer_set_td_bootstrap(xq_trainer* t, int kind);
/* xq_dqn_set_zero_sum on the trainer's Q-net (DESIGN.md §4 "Zero-sum target").  Uniform, prioritized and on-policy rings, any n_step,
 * overlap_collect 0 and 1; no window changes.  The zero-sum target is for transitions whose s' has the other side to decide, and a
 * versus transition runs from one learner decision to the next: on = 1 while an opponent is set is XQ_ERR_INVALID_ARGUMENT, and so is
 * xq_trainer_set_opponent(non-NULL) while zero-sum is on.  Call between iterations: XQ_ERR_RUNTIME while a learn_grads waits for its
 * learn_apply. */
int xq_trainer_set_zero_sum(xq_trainer* t, int on);
/* The mover view (DESIGN.md §4 "Mover view") on the trainer: xq_dqn_set_view on its Q-net, xq_env_set_q_view on its env, and both side
 * columns on its ring (xq_replay_track_mover, xq_replay_track_next_player).  Before the first collect (XQ_ERR_RUNTIME afterwards: the
 * columns need an empty ring).  Every collect then stages view(board, side to move) of the env's boards with view_boards_kernel on the
 * collect's stream and hands that to the select chain; a versus NET opponent is read through ITS OWN handle's view.  Composes with
 * zero-sum, both bootstraps, n-step, mirror, prioritized replay and overlap_collect 0 and 1; with xq_trainer_set_colour_swap(prob > 0)
 * learn_grads is XQ_ERR_INVALID_ARGUMENT. */
int xq_trainer_set_view(xq_trainer* t, int view);
/* Versus training (DESIGN.md §4 "Versus training"): from the next collect on, the learner plays against a fixed opponent instead of
 * itself — uniform-random play, the material search (depth 1..3, eps) or a borrowed network (eps; layer_sizes[0] == 1260, >= 90
 * outputs, not the trainer's own).  The learner plays Black in game g iff (first_game_id + g) & 1.  A collect still writes one
 * transition per game, from one learner decision to the next: the opponent moves first where it is to move (a game it ends there gives
 * an empty slot), then the learner, then the opponent's reply; reward = evaluateBoard(learner, moveCount) at s'.  The borrowed network's
 * forwards run on its own stream (ordered by events), keep no layer-0 sums and touch no TD-step state.  NULL returns to self-play.
 * Call between iterations.  A bad kind, depth or eps, a NULL dqn for XQ_PLAYER_NET or a network of the wrong shape: INVALID_ARGUMENT. */
int xq_trainer_set_opponent(xq_trainer* t, const xq_arena_player* opp);
/* Learner wins, draws, losses and games ended since the last xq_trainer_set_opponent (the arena's rules: the captor of a general wins,
 * the side without a legal move loses, the 200-move cap is a draw). */
int xq_trainer_versus_results(xq_trainer* t, uint64_t out[4]);
int xq_trainer_collect(xq_trainer* t);                       /* one ply in every game */
int xq_trainer_learn_grads(xq_trainer* t);                   /* sample + gradients into the grad buffer */
int xq_trainer_learn_apply(xq_trainer* t, int world_size);   /* SGD apply (+ target sync bookkeeping) */
int xq_trainer_step(xq_trainer* t, int n_iterations);        /* (collect x collects_per_update) + learn_grads + learn_apply(world of the attached communicator, else 1), n times */
int xq_trainer_counters(xq_trainer* t, uint64_t* env_steps, uint64_t* updates, uint64_t* episodes);

#ifdef __cplusplus
}
#endif
#endif /* XQ_CAPI_H */
