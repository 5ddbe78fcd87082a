// xq_stage.hip.h — the staging transforms of a TD step from a ring (DESIGN.md §4 "Staging pipeline"): mirror augmentation
// (xq_replay_set_mirror: col -> 8 - col), colour-swap augmentation (xq_replay_set_colour_swap: row -> 9 - row, Red <-> Black) and the
// mover-relative view (xq_dqn_set_view: the colour swap of a board whose side to move is Black).  Each rewrites both boards and the
// action's square of a minibatch row in the handle's staging batch, on which the TD step then runs unchanged; the ring is never
// written.  One row routine (stage_load, stage_store<Map>) serves the three kernels, which add only where their flags come from and
// what they do with the side bytes; view_boards_kernel maps packed boards with a side each.
// (kernel half of xq_dqn.hip; included by xq_dqn.hip only, behind xq_l0.hip.h for SlotSrc / slot_of and beside xq_nstep.hip.h)
#pragma once

namespace xq {

// A board is 96 nibbles in 12 words, square s = nibble s & 7 of word s >> 3, so board row r is the 36 bits from bit 36 r: it starts at
// nibble phase r mod 8 and straddles two words (rows 0-7: words r, r + 1; row 8: 9, 10; row 9: 10, 11).  Both maps cut each row out of
// the 64-bit window of its two words, shifted and masked to 36 bits, and OR its image into zeroed words, so nibbles 90..95 come out 0.
// Fully unrolled: every word index and shift is a compile-time constant (a register array indexed at run time would go to scratch).

// Left-right reflection.  Per row: its nine nibbles reversed (byte swap, the nibbles of each byte swapped: sixteen nibbles reversed,
// nibble i -> 15 - i; down by 7 nibbles: i -> 8 - i), back at the row's own phase.
struct MirrorMap {
    static __device__ __forceinline__ void board(const uint32_t (&w)[kBoardWords], uint32_t (&o)[kBoardWords]) {
#pragma unroll
        for (int i = 0; i < kBoardWords; ++i) o[i] = 0u;
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const int wi = (36 * r) >> 5, sh = (36 * r) & 31;
            const uint64_t win = (uint64_t)w[wi] | ((uint64_t)w[wi + 1] << 32);
            const uint64_t x = (win >> sh) & 0xFFFFFFFFFull;
            uint64_t y = __builtin_bswap64(x);
            y = ((y & 0x0F0F0F0F0F0F0F0Full) << 4) | ((y >> 4) & 0x0F0F0F0F0F0F0F0Full);
            y = (y >> 28) << sh;             // (sh <= 28: the 36 bits stay inside the window)
            o[wi] |= (uint32_t)y;
            o[wi + 1] |= (uint32_t)(y >> 32);
        }
    }
    static __device__ __forceinline__ int square(int a) { return a - 2 * (a % 9) + 8; }          // (row, 8 - col) of a square 0..89
};

// sigma on the eight nibbles of a word at once: 0 stays, 1..7 (Red) + 7, 8..14 (Black) - 7.  `hi` holds a 1 at the bottom of every nibble
// whose high bit is set, `nz` at every non-zero nibble; neither step carries across a nibble (7 + 7 = 14, 8 - 7 = 1).
__device__ __forceinline__ uint32_t colour_swap_codes(uint32_t x) {
    const uint32_t hi = (x >> 3) & 0x11111111u;
    const uint32_t nz = (x | (x >> 1) | (x >> 2) | (x >> 3)) & 0x11111111u;
    return x + 7u * (nz & ~hi) - 7u * hi;
}

// Colour exchange with the board turned top to bottom.  Row r of the image is row 9 - r of sigma(board): the 36-bit field is cut out at
// nibble phase r mod 8 and ORed in at the phase of 9 - r.
struct ColourSwapMap {
    static __device__ __forceinline__ void board(const uint32_t (&w)[kBoardWords], uint32_t (&o)[kBoardWords]) {
        uint32_t c[kBoardWords];
#pragma unroll
        for (int i = 0; i < kBoardWords; ++i) { c[i] = colour_swap_codes(w[i]); o[i] = 0u; }
#pragma unroll
        for (int r = 0; r < 10; ++r) {
            const int wi = (36 * r) >> 5, sh = (36 * r) & 31;
            const int wo = (36 * (9 - r)) >> 5, so = (36 * (9 - r)) & 31;
            const uint64_t win = (uint64_t)c[wi] | ((uint64_t)c[wi + 1] << 32);
            const uint64_t y = ((win >> sh) & 0xFFFFFFFFFull) << so;       // (so <= 28: the 36 bits stay inside the window)
            o[wo] |= (uint32_t)y;
            o[wo + 1] |= (uint32_t)(y >> 32);
        }
    }
    static __device__ __forceinline__ int square(int a) { return a + 81 - 18 * (a / 9); }        // (9 - row, col) of a square 0..89
};

struct BoardRegs { uint4 q0, q1, q2; };          // a packed board as loaded: three 16-byte pieces (48 B slots of hipMalloc'ed arrays)

__device__ __forceinline__ BoardRegs board_load(const uint32_t* boards, long long i) {
    const uint4* p = reinterpret_cast<const uint4*>(boards + i * kBoardWords);
    return BoardRegs{p[0], p[1], p[2]};
}

// Map(board) where `flag`, the board itself elsewhere: transformed unconditionally and selected by the flag, so no wave diverges on it
template <class Map>
__device__ __forceinline__ void board_store(uint32_t* out, long long i, const BoardRegs& q, bool flag) {
    const uint32_t w[kBoardWords] = {q.q0.x, q.q0.y, q.q0.z, q.q0.w, q.q1.x, q.q1.y, q.q1.z, q.q1.w, q.q2.x, q.q2.y, q.q2.z, q.q2.w};
    const uint32_t keep = flag ? 0u : 0xFFFFFFFFu;
    uint32_t o[kBoardWords];
    Map::board(w, o);
#pragma unroll
    for (int k = 0; k < kBoardWords; ++k) o[k] = (w[k] & keep) | (o[k] & ~keep);
    uint4* p = reinterpret_cast<uint4*>(out + i * kBoardWords);
    p[0] = make_uint4(o[0], o[1], o[2], o[3]); p[1] = make_uint4(o[4], o[5], o[6], o[7]); p[2] = make_uint4(o[8], o[9], o[10], o[11]);
}

// What every staging transform reads and writes.  gather (uniform over the launch): from the ring at the sampled slot into the staging
// batch, with reward, done and the slot; otherwise the staging batch in place, by row (the source pointers are the staged ones; reward,
// done, the slot and the n-step row fields are left alone)
struct StageIo {
    const uint32_t* boards; const uint32_t* next_boards; const int32_t* action_to; const float* reward; const uint8_t* done;
    uint32_t* s_boards; uint32_t* s_next; int32_t* s_action; float* s_reward; uint8_t* s_done; int32_t* s_first;
    uint32_t gather;
};

// The Philox words of a random transform: flag_b = all || philox(b, 0, call, stream_word).v[0] < thresh
struct StageDraw { uint32_t thresh, all, call, seed_lo, seed_hi; };

__device__ __forceinline__ bool flag_of(const StageDraw& dr, int b, uint32_t stream_word) {
    return dr.all != 0u || philox4x32_10((uint32_t)b, 0u, dr.call, stream_word, dr.seed_lo, dr.seed_hi).v[0] < dr.thresh;
}

struct StageRow { int s; BoardRegs brd, nxt; int a; float rw; uint8_t dn; };

// What row b reads: the sampled slot of the ring (slot_of: nstep_assemble_kernel's layout), or in place the row itself
__device__ __forceinline__ int stage_slot(const StageIo& io, const SlotSrc& src, int b) { return io.gather != 0u ? slot_of(src, b) : b; }

// One thread per row.  Every load of the row — six 16-byte board loads, the action and, in the gather form, reward and done — is
// issued before the first use, so a thread has read its whole row before it writes any of it (in place the rows it reads are the rows
// it writes)
__device__ __forceinline__ StageRow stage_load(const StageIo& io, int s) {
    StageRow row;
    row.s = s;
    row.brd = board_load(io.boards, row.s);
    row.nxt = board_load(io.next_boards, row.s);
    row.a = io.action_to[row.s];
    row.rw = 0.f; row.dn = 0;
    if (io.gather != 0u) { row.rw = io.reward[row.s]; row.dn = io.done[row.s]; }
    return row;
}

// Row b of the staging batch: s mapped where flag_s, s' where flag_next, the action's square with s (anything but a square 0..89 stays:
// -1 of a dead or empty row, 90..95)
template <class Map>
__device__ __forceinline__ void stage_store(const StageIo& io, int b, const StageRow& row, bool flag_s, bool flag_next) {
    board_store<Map>(io.s_boards, b, row.brd, flag_s);
    board_store<Map>(io.s_next, b, row.nxt, flag_next);
    io.s_action[b] = (flag_s && row.a >= 0 && row.a < 90) ? Map::square(row.a) : row.a;
    if (io.gather != 0u) { io.s_reward[b] = row.rw; io.s_done[b] = row.dn; io.s_first[b] = row.s; }
}

struct MirrorArgs {
    StageIo io;
    StageDraw draw;                          // stream word 3
    uint8_t* s_flag;
};

__global__ __launch_bounds__(64) void mirror_stage_kernel(MirrorArgs A, SlotSrc src, int batch) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= batch) return;
    const StageRow row = stage_load(A.io, stage_slot(A.io, src, b));
    const bool flag = flag_of(A.draw, b, 3u);
    stage_store<MirrorMap>(A.io, b, row, flag, flag);
    A.s_flag[b] = flag ? (uint8_t)1 : (uint8_t)0;
}

struct ColourSwapArgs {
    StageIo io;
    StageDraw draw;                          // stream word 4
    uint8_t* s_flag;
    // legal-move bootstrap only (ring_side == nullptr: no side is staged): s_side[b] = flag_b ? 1 - ring_side[slot] : ring_side[slot], the slot from
    // row_slot[b] (in place: the slot whose side the staged row takes) or, with row_slot == nullptr, the gathered slot itself
    const uint8_t* ring_side; const int32_t* row_slot; uint8_t* s_side;
    int cap;
};

// The side's slot is loaded with the row; only the side byte, whose address is that slot, follows
__global__ __launch_bounds__(64) void colour_swap_stage_kernel(ColourSwapArgs A, SlotSrc src, int batch) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= batch) return;
    const bool sided = A.ring_side != nullptr;
    const int s = stage_slot(A.io, src, b);
    int ss = s;
    if (sided && A.row_slot) ss = A.row_slot[b];
    const StageRow row = stage_load(A.io, s);
    uint8_t sd = 0;
    if (sided && (unsigned)ss < (unsigned)A.cap) sd = A.ring_side[ss];
    const bool flag = flag_of(A.draw, b, 4u);
    stage_store<ColourSwapMap>(A.io, b, row, flag, flag);
    A.s_flag[b] = flag ? (uint8_t)1 : (uint8_t)0;
    if (sided) A.s_side[b] = flag ? (uint8_t)(1 - sd) : sd;
}

struct MoverViewArgs {
    StageIo io;
    // the ring's two side columns, by slot: flag_s = mover[first slot], flag_s' = next_player[the slot whose s' was staged].  In place
    // the two slots are row_first[b] and row_last[b] (behind the n-step assembly its first and last slot; behind the mirror alone both are
    // the sampled slot); the gather form takes the gathered slot for both and reads neither array
    const uint8_t* mover; const uint8_t* next_player; const int32_t* row_first; const int32_t* row_last;
    uint8_t* s_flag; uint8_t* s_flag_next;   // the two flags, per row
    uint8_t* s_side;                         // legal-move bootstrap only (else nullptr): the staged side to move in s' — 0, Red, on every row
    int cap;
};

// The last staging transform: s by who moved, s' by who moves next, the action with s.  In place the two slots are loaded with the row;
// only the two side bytes, whose addresses are the slots, follow
__global__ __launch_bounds__(64) void mover_view_stage_kernel(MoverViewArgs A, SlotSrc src, int batch) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= batch) return;
    const int s = stage_slot(A.io, src, b);
    int sf = s, sl = s;
    if (A.io.gather == 0u) { sf = A.row_first[b]; sl = A.row_last[b]; }
    const StageRow row = stage_load(A.io, s);
    uint8_t mv = 0, np = 0;
    if ((unsigned)sf < (unsigned)A.cap) mv = A.mover[sf];
    if ((unsigned)sl < (unsigned)A.cap) np = A.next_player[sl];
    stage_store<ColourSwapMap>(A.io, b, row, mv != 0, np != 0);
    A.s_flag[b] = mv != 0 ? (uint8_t)1 : (uint8_t)0;
    A.s_flag_next[b] = np != 0 ? (uint8_t)1 : (uint8_t)0;
    if (A.s_side != nullptr) A.s_side[b] = 0;
}

// view(board, side): the board when Red is to move and its colour swap when Black is.  One thread per board; the three 16-byte loads
// and the side are issued before the first use.  The side of board b is side[b] != 0 or, with meta != nullptr (uniform over the launch:
// the boards are an env's), bit 16 of meta[b].x.  Nibbles 90..95 come out 0 on the swapped boards and as they were on the others.
__global__ __launch_bounds__(64) void view_boards_kernel(const uint32_t* __restrict__ boards, const uint8_t* __restrict__ side,
                                                         const uint4* __restrict__ meta, int n, uint32_t* __restrict__ out) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n) return;
    const BoardRegs q = board_load(boards, b);
    const bool black = meta != nullptr ? ((meta[b].x >> 16) & 1u) != 0u : side[b] != 0;
    board_store<ColourSwapMap>(out, b, q, black);
}

}  // namespace xq
