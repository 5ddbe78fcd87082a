// xq_search.hip — fixed-depth full-width material negamax over the env's move lists (DESIGN.md §4 "Search player"), on gfx950.
//
// One 256-thread block per board.  Every wave unpacks the board into an LDS slab of its own and generates the root list there
// (gen_all_actions, the canonical getAllValidActions order); the list is then held in two VGPRs (lane, 64 + lane) so that the slab's
// move array is free for the replies.  The four waves take the root moves in a strided loop: a wave applies its move to its own board
// copy, searches below it with gen_all_actions + a wave maximum per node, and undoes the move (two byte writes).  At depth 3 the wave
// walks the reply list sequentially and applies each reply to a second slab.  The root values meet in LDS and wave 0 reduces them.
// Nothing below the root is kept: the value of a child is the captured piece's value minus the value of the position below it, so no
// node scans the board.
//
// Why a block per board rather than a wave per (board, root move): it needs no launch to build the root lists first, the root list
// never goes through HBM, and a board's ~40 root moves keep 4 waves busy for a similar time (the strided loop balances them to within
// one move).  8192 boards give 32 k waves, several times the 8 k wave slots of the device, so occupancy is not the limit.
#include "xq_internal.h"
#include "xq_rules.hip.h"

#include <climits>

namespace xq {
namespace {

constexpr int kMate = XQ_SEARCH_MATE;
constexpr int kWaves = 4;

struct SearchParams {
    const uint32_t* boards;
    const uint4* meta;
    int first;                      // games [first, first + gridDim.x) of the env
    // analysis: [n][128] root values (INT_MIN past the count), the move count and the first best index (-1: no move), per game
    int32_t* values;
    int32_t* counts;
    int32_t* best;
    // arena pick: one index into the game's move list; frozen games are skipped
    int16_t* pick;
    uint32_t eps_u32, seed_lo, seed_hi, first_game_id;
    int pairs;                      // twins g and g + pairs share the tie-break stream
};

__device__ __forceinline__ int wave_max_i32(int v) {                  // maximum over the 64 lanes, wave-uniform (DPP as wave_max)
    auto step = [&](int t) { v = v > t ? v : t; };
    step(dpp_int<0x111, 0xf>(INT_MIN, v));
    step(dpp_int<0x112, 0xf>(INT_MIN, v));
    step(dpp_int<0x114, 0xf>(INT_MIN, v));
    step(dpp_int<0x118, 0xf>(INT_MIN, v));
    step(dpp_int<0x142, 0xa>(INT_MIN, v));
    step(dpp_int<0x143, 0xc>(INT_MIN, v));
    return __builtin_amdgcn_readlane(v, 63);
}

// value of the piece a move lands on, for a child k + 1 plies from the root: a general ends the game there
__device__ __forceinline__ int capture_value(int victim, int k) {
    return code_type(victim) == T_GENERAL ? kMate - (k + 1) : piece_value(victim);
}

// movePiece on the wave's board (code wave-uniform, the move generated on this board): returns the victim; undo_move restores
__device__ __forceinline__ int do_move(uint8_t* sq, int code) {
    const int from = code / 90, to = code - from * 90;
    const int moving = __builtin_amdgcn_readfirstlane((int)sq[from]);
    const int victim = __builtin_amdgcn_readfirstlane((int)sq[to]);
    wave_sync();
    if (lane_id() == 0) { sq[to] = (uint8_t)moving; sq[from] = 0; }
    wave_sync();
    return victim;
}
__device__ __forceinline__ void undo_move(uint8_t* sq, int code, int victim) {
    const int from = code / 90, to = code - from * 90;
    const int moving = __builtin_amdgcn_readfirstlane((int)sq[to]);
    wave_sync();
    if (lane_id() == 0) { sq[from] = (uint8_t)moving; sq[to] = (uint8_t)victim; }
    wave_sync();
}

// N(pos, side, k, 1): the best capture value of side's list, -(MATE - k) without a move
__device__ int negamax1(WaveSlab& S, int side, int k) {
    const int n = gen_all_actions(S, side);
    wave_sync();
    if (n == 0) return -(kMate - k);
    const int lane = lane_id();
    int v = INT_MIN;
    if (lane < n) v = capture_value(S.sq[S.moves[lane] % 90], k);
    if (lane + 64 < n) { const int v1 = capture_value(S.sq[S.moves[lane + 64] % 90], k); v = v > v1 ? v : v1; }
    return wave_max_i32(v);
}

// N(pos, side, k, 2): the replies are generated on A (whose board is pos) and each is played on B, a copy of A's board
__device__ int negamax2(WaveSlab& A, WaveSlab& B, int side, int k) {
    const int n = gen_all_actions(A, side);
    wave_sync();
    if (n == 0) return -(kMate - k);
    const int lane = lane_id();
    if (lane < kBoardWords * 2) reinterpret_cast<uint32_t*>(B.sq)[lane] = reinterpret_cast<const uint32_t*>(A.sq)[lane];
    wave_sync();
    int best = INT_MIN;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const int code = __builtin_amdgcn_readfirstlane((int)A.moves[i]);
        const int victim = __builtin_amdgcn_readfirstlane((int)B.sq[code % 90]);
        int child;
        if (code_type(victim) == T_GENERAL) {
            child = kMate - (k + 1);
        } else {
            do_move(B.sq, code);
            child = piece_value(victim) - negamax1(B, side ^ 1, k + 1);
            undo_move(B.sq, code, victim);
        }
        best = best > child ? best : child;
    }
    return best;
}

// SEATED (versus training, PICK only): a block searches only where the learner's opponent is to move — the learner plays Black in game g
// iff (first_game_id + g) & 1 — and the game's versus slot of this collect is not written yet (kMetaVsDone)
template <int DEPTH, bool PICK, bool SEATED = false>
__global__ __launch_bounds__(256) void search_kernel(SearchParams P) {
    __shared__ WaveSlab slabs[kWaves][DEPTH == 3 ? 2 : 1];
    __shared__ int32_t root_val[kMaxMoves];
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = lane_id();
    const int g = P.first + (int)blockIdx.x;
    WaveSlab& S = slabs[wid][0];

    uint4 m = P.meta[g];
    m.x = __builtin_amdgcn_readfirstlane(m.x);
    m.z = __builtin_amdgcn_readfirstlane(m.z);
    if (PICK && (m.x & kMetaFrozen)) return;                       // (block-uniform: every wave reads the same meta)
    if (SEATED && (((m.x >> 16) & 1u) == ((P.first_game_id + (uint32_t)g) & 1u) || (m.x & kMetaVsDone))) return;
    const int side = (int)((m.x >> 16) & 1u);
    const uint32_t plies = m.z;
    const uint32_t word = lane < kBoardWords ? P.boards[(size_t)g * kBoardWords + lane] : 0u;
    unpack_to_slab(word, S.sq);
    wave_sync();
    const int n = gen_all_actions(S, side);
    wave_sync();
    const int rm0 = lane < n ? (int)S.moves[lane] : 0;             // the root list, out of the slab's way
    const int rm1 = lane + 64 < n ? (int)S.moves[lane + 64] : 0;

    bool explore = false;
    Philox4 r{{0u, 0u, 0u, 0u}};
    if (PICK && n > 0) {                                            // the env kernel's own epsilon draw (<SELFPLAY>): an exploring
        r = philox4x32_10(plies, 0u, P.first_game_id + (uint32_t)g, 0u, P.seed_lo, P.seed_hi);   // game is not searched
        explore = r.v[0] < P.eps_u32;
    }
    if (!explore) {
#pragma unroll 1
        for (int i = wid; i < n; i += kWaves) {
            const int code = i < 64 ? __builtin_amdgcn_readlane(rm0, i) : __builtin_amdgcn_readlane(rm1, i - 64);
            const int victim = __builtin_amdgcn_readfirstlane((int)S.sq[code % 90]);
            int v = capture_value(victim, 0);
            if constexpr (DEPTH > 1) {
                if (code_type(victim) != T_GENERAL) {                // (a general capture ends the game: nothing below it)
                    do_move(S.sq, code);
                    if constexpr (DEPTH == 2) v -= negamax1(S, side ^ 1, 1);
                    else v -= negamax2(S, slabs[wid][1], side ^ 1, 1);
                    undo_move(S.sq, code, victim);
                }
            }
            if (lane == 0) root_val[i] = v;
        }
    }
    __syncthreads();
    if (wid != 0) return;

    const int v0 = lane < n && !explore ? root_val[lane] : INT_MIN;
    const int v1 = lane + 64 < n && !explore ? root_val[lane + 64] : INT_MIN;
    const int top0 = wave_max_i32(v0), top1 = wave_max_i32(v1);
    const int top = top0 > top1 ? top0 : top1;
    const unsigned long long b0 = __ballot(lane < n && v0 == top), b1 = __ballot(lane + 64 < n && v1 == top);
    if (!PICK) {
        int32_t* vals = P.values + (size_t)(g - P.first) * kMaxMoves;
        vals[lane] = v0;
        vals[lane + 64] = v1;
        if (lane == 0) {
            P.counts[g - P.first] = n;
            P.best[g - P.first] = b0 ? __ffsll((long long)b0) - 1 : (b1 ? 63 + __ffsll((long long)b1) : -1);
        }
        return;
    }
    int idx = 0;
    if (n > 0 && explore) {
        idx = (int)(r.v[1] % (uint32_t)n);
    } else if (n > 0) {                                             // the (r0 % n_best)-th best in list order, on the PAIR's stream
        const int twin = g >= P.pairs ? g - P.pairs : g;
        const Philox4 t = philox4x32_10(plies, 0u, P.first_game_id + (uint32_t)twin, 3u, P.seed_lo, P.seed_hi);
        const int c0 = __popcll(b0), n_best = c0 + __popcll(b1);
        const int j = (int)(t.v[0] % (uint32_t)n_best);
        const unsigned long long mask = j < c0 ? b0 : b1;
        const int jj = j < c0 ? j : j - c0;
        const unsigned long long below = (1ull << lane) - 1ull;
        const unsigned long long hit = __ballot(((mask >> lane) & 1ull) && __popcll(mask & below) == jj);
        idx = (j < c0 ? 0 : 64) + __ffsll((long long)hit) - 1;
    }
    if (lane == 0) P.pick[g] = (int16_t)idx;
}

template <int DEPTH, bool PICK, bool SEATED = false>
int launch_depth(const SearchParams& P, int n_boards, hipStream_t s) {
    hipLaunchKernelGGL((search_kernel<DEPTH, PICK, SEATED>), dim3(n_boards), dim3(64 * kWaves), 0, s, P);
    XQ_HIP(hipGetLastError());
    return XQ_OK;
}

template <bool PICK, bool SEATED = false>
int launch(const SearchParams& P, int depth, int n_boards, hipStream_t s) {
    if (n_boards <= 0) return XQ_OK;
    switch (depth) {
        case 1: return launch_depth<1, PICK, SEATED>(P, n_boards, s);
        case 2: return launch_depth<2, PICK, SEATED>(P, n_boards, s);
        case 3: return launch_depth<3, PICK, SEATED>(P, n_boards, s);
        default: return fail(XQ_ERR_INVALID_ARGUMENT, "search depth must be 1, 2 or 3 (got %d)", depth);
    }
}

SearchParams base(const xq_env* e, int first) {
    SearchParams P;
    memset(&P, 0, sizeof P);
    P.boards = e->boards;
    P.meta = e->meta;
    P.first = first;
    P.seed_lo = (uint32_t)e->seed;
    P.seed_hi = (uint32_t)(e->seed >> 32);
    P.first_game_id = e->first_id;
    return P;
}

}  // namespace

// The search player's picks for games [first, first + count) of e on stream s (xq_internal.h).  seated: ties are broken on the game's
// own stream (ctr {plies, 0, first_game_id + g, 3}: no twin); the epsilon draw is the env kernel's either way
int search_pick_launch(xq_env* e, int depth, int first, int count, int pairs, bool seated, uint32_t eps_u32, int16_t* pick_dev, hipStream_t s) {
    SearchParams P = base(e, first);
    P.pick = pick_dev;
    P.eps_u32 = eps_u32;
    P.pairs = pairs;
    return !seated ? launch<true>(P, depth, count, s) : launch<true, true>(P, depth, count, s);
}

}  // namespace xq

using namespace xq;

extern "C" {

int xq_env_search_dev(xq_env* e, int depth, int32_t* values_dev, int32_t* counts_dev, int32_t* best_dev) {
    if (!e || !values_dev || !counts_dev || !best_dev) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_env_search: null pointer");
    if (depth < 1 || depth > 3) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_env_search: depth must be 1, 2 or 3 (got %d)", depth);
    SearchParams P = base(e, 0);
    P.values = values_dev;
    P.counts = counts_dev;
    P.best = best_dev;
    return launch<false>(P, depth, e->n, e->stream);
}

int xq_env_search(xq_env* e, int depth, int32_t* values_host, int32_t* counts_host, int32_t* best_host) {
    if (!e || !values_host || !counts_host || !best_host) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_env_search: null pointer");
    if (depth < 1 || depth > 3) return fail(XQ_ERR_INVALID_ARGUMENT, "xq_env_search: depth must be 1, 2 or 3 (got %d)", depth);
    const size_t n = (size_t)e->n;
    DevBuf<int32_t> buf;
    XQ_TRY(buf.alloc(n * (kMaxMoves + 2)));
    int rc = xq_env_search_dev(e, depth, buf, buf + n * kMaxMoves, buf + n * (kMaxMoves + 1));
    hipError_t he = hipSuccess;
    if (rc == XQ_OK) he = hipMemcpyAsync(values_host, buf, n * kMaxMoves * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    if (rc == XQ_OK && he == hipSuccess) he = hipMemcpyAsync(counts_host, buf + n * kMaxMoves, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    if (rc == XQ_OK && he == hipSuccess) he = hipMemcpyAsync(best_host, buf + n * (kMaxMoves + 1), n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream);
    const hipError_t hs = hipStreamSynchronize(e->stream);        // (the copies out of buf are done, or failed, before it goes)
    if (rc != XQ_OK) return rc;
    XQ_HIP(he);
    XQ_HIP(hs);
    return XQ_OK;
}

}  // extern "C"
